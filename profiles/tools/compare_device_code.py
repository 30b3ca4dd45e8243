#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of libptnn.so, object by object and kernel by kernel (needs no GPU).

    python3 profiles/tools/compare_device_code.py OLD_BUILD_DIR NEW_BUILD_DIR

Each argument is a csrc/build/ directory that __graft_entry__.build() filled (the *.o files).  For every object the gfx950 code
object is taken out of its .hip_fatbin section (llvm-objcopy, clang-offload-bundler); for every kernel in it the instruction bytes
(llvm-objdump -d) and the metadata entry of the kernel (llvm-readelf --notes: registers, LDS, scratch, kernel arguments) are
compared with the kernel of the same name in the other build, in whichever object it sits there.  Exit status 0: every kernel
of either build exists in the other with identical bytes and metadata.  Whole code objects are compared too, section by section (see NAME_TABLES)."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/lib/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def run(tool, *args):
    return subprocess.run([os.path.join(LLVM, tool), *args], check=True, capture_output=True, text=True).stdout


def code_object(obj, tmp):
    """The gfx950 code object of a host object file, or None when it has no device code."""
    bundle, co = os.path.join(tmp, "bundle"), os.path.join(tmp, "co")
    for f in (bundle, co):
        if os.path.exists(f):
            os.remove(f)
    if ".hip_fatbin" not in run("llvm-readelf", "-S", obj):     # a host-only object (checkpoint, text)
        return None
    run("llvm-objcopy", "--dump-section", ".hip_fatbin=" + bundle, obj, os.path.join(tmp, "unused.o"))
    run("clang-offload-bundler", "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + bundle, "--output=" + co)
    return co if os.path.getsize(co) else None


def kernels_of(co):
    """{kernel name: (instruction bytes as text, metadata entry)} of one code object."""
    meta = {}
    entry = None
    for line in run("llvm-readelf", "--notes", co).splitlines():
        if re.match(r"\s*amdhsa\.kernels:", line):
            entry = []
        elif entry is not None and re.match(r"\s*amdhsa\.\w+:", line):      # the next top-level key ends the kernel list
            break
        elif entry is not None:
            entry.append(line)
    for text in re.split(r"\n(?= {2}- )", "\n".join(entry or [])):
        name = re.search(r"^\s+\.name:\s+(\S+)", text, re.M)
        if name:
            meta[name.group(1)] = text
    size = {}                                   # bytes of every function: the disassembly of the last one runs on into the section's padding
    for line in run("llvm-readelf", "-sW", co).splitlines():
        f = line.split()
        if len(f) == 8 and f[3] == "FUNC":
            size[f[7]] = int(f[2], 0)
    code, sym = {}, None
    for line in run("llvm-objdump", "-d", co).splitlines():
        m = re.match(r"[0-9a-f]+ <(.+)>:$", line)
        if m:
            sym = m.group(1)
            code[sym] = []
        elif sym and "//" in line:
            code[sym] += line.split("//")[1].split(":", 1)[1].split()       # "ADDRESS: WORDS" -> the 32-bit words
    return {k: (" ".join(code[k][:size[k] // 4]), meta[k]) for k in meta}


# One thing in a code object names where it was built: the dynamic symbol __hip_cuid_<hash>, the compilation unit's id, a hash of
# the source path and the command line.  Its name decides these tables (order, buckets, strings; .dynamic and .symtab hold their
# addresses and sizes); every other section -- .text, .rodata, .note with the kernels' metadata, relocations -- is compared.
NAME_TABLES = (".dynsym", ".gnu.hash", ".hash", ".dynstr", ".strtab", ".dynamic", ".symtab")


def sections_digest(co, tmp):
    h = hashlib.sha256()
    for line in run("llvm-readelf", "-SW", co).splitlines():
        m = re.match(r"\s*\[\s*\d+\]\s+(\.\S+)\s+(\S+)", line)
        if m and m.group(2) != "NOBITS" and m.group(1) not in NAME_TABLES:
            part = os.path.join(tmp, "section")
            run("llvm-objcopy", "--dump-section", m.group(1) + "=" + part, co, os.path.join(tmp, "unused.co"))
            h.update(m.group(1).encode() + open(part, "rb").read())
    return h.hexdigest()


def scan(build_dir):
    objects, found = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for name in sorted(os.listdir(build_dir)):
            if not name.endswith(".o"):
                continue
            co = code_object(os.path.join(build_dir, name), tmp)
            if co is None:
                objects[name] = None
                continue
            objects[name] = sections_digest(co, tmp)
            for k, v in kernels_of(co).items():
                found.setdefault(k, []).append((name, v))
    # a kernel's name carries its template arguments (T, I, O): a kernel that moved is matched by it; only a name that several objects of one build define is keyed by its object too
    return objects, {(k, name if len(at) > 1 else ""): (name, v) for k, at in found.items() for name, v in at}


def main():
    old_o, old_k = scan(sys.argv[1])
    new_o, new_k = scan(sys.argv[2])
    same = [n for n in old_o if n in new_o and old_o[n] == new_o[n] and old_o[n] is not None]
    print(f"objects: {len(old_o)} old, {len(new_o)} new; code objects with identical sections: {len(same)} ({', '.join(same)})")
    bad = 0
    for key in sorted(set(old_k) | set(new_k)):
        if key not in old_k or key not in new_k:
            print(f"ONLY IN {'OLD' if key in old_k else 'NEW'}: {key[0]} ({(old_k.get(key) or new_k.get(key))[0]})")
            bad += 1
            continue
        (oo, (oc, om)), (no, (nc, nm)) = old_k[key], new_k[key]
        what = [w for w, a, b in (("instructions", oc, nc), ("metadata", om, nm)) if a != b]
        if what:
            print(f"DIFFERENT {' and '.join(what)}: {key[0]} ({oo} -> {no})")
            bad += 1
        elif oo != no:
            print(f"moved, identical: {key[0]} ({oo} -> {no})")
    print(f"kernels: {len(old_k)} old, {len(new_k)} new, {bad} differ or are missing")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
