// Micro-benchmark (diagnostic, not the product): what does each instruction of the hand-scheduled SGD row (ptnn_dev_math.hpp:
// PTNN_SW_STEP) cost ONE wave that is alone on its CU, in a long stream?  The row loop's budget is counted in issue slots of 4
// cycles; this measures the slots: plain and packed FMAs in the two operand forms the loop uses, the transcendentals, the DPP add
// behind its two hazard slots, the scalar row fetch (s_load_dwordx8 per row against s_load_dwordx16 per two rows, each with its
// s_waitcnt one row of VALU later) and the loop control.
//   hipcc --offload-arch=gfx950 -O3 -o sweep_issue_costs sweep_issue_costs.hip && ./sweep_issue_costs [iters]
// One work-group of one wave.  Timed with s_memrealtime (100 MHz, the counter ptnn_time_sgd_epoch uses) and, beside it, s_memtime
// (shader cycles): cycles per instruction come from the second, the clock the wave ran at from the ratio of the two.
// Every stream is a counted loop; cost per unit = (T(body of 2N units) - T(body of N units)) / (N iters), so the loop's own
// instructions cancel.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>

typedef unsigned long long u64;

#define FMA8 \
    "v_fma_f32 v40, v56, s36, v40\n v_fma_f32 v41, v56, s36, v41\n v_fma_f32 v42, v56, s36, v42\n v_fma_f32 v43, v56, s36, v43\n" \
    "v_fma_f32 v44, v56, s36, v44\n v_fma_f32 v45, v56, s36, v45\n v_fma_f32 v46, v56, s36, v46\n v_fma_f32 v47, v56, s36, v47\n"
#define FMA24 FMA8 FMA8 FMA8
#define FMA25 FMA24 "v_fma_f32 v48, v56, s36, v48\n"
// (v_pk_fma_f32 reads its scalar pair from s[52:53]: no load of this file writes it)
#define PKS4 \
    "v_pk_fma_f32 v[40:41], s[52:53], v[56:57], v[40:41]\n v_pk_fma_f32 v[42:43], s[52:53], v[56:57], v[42:43]\n" \
    "v_pk_fma_f32 v[44:45], s[52:53], v[56:57], v[44:45]\n v_pk_fma_f32 v[46:47], s[52:53], v[56:57], v[46:47]\n"
#define PKO4 \
    "v_pk_fma_f32 v[40:41], v[56:57], s[52:53], v[40:41] op_sel_hi:[0,1,1]\n v_pk_fma_f32 v[42:43], v[56:57], s[52:53], v[42:43] op_sel_hi:[0,1,1]\n" \
    "v_pk_fma_f32 v[44:45], v[56:57], s[52:53], v[44:45] op_sel_hi:[0,1,1]\n v_pk_fma_f32 v[46:47], v[56:57], s[52:53], v[46:47] op_sel_hi:[0,1,1]\n"
#define EXP4 "v_exp_f32_e32 v40, v56\n v_exp_f32_e32 v41, v56\n v_exp_f32_e32 v42, v56\n v_exp_f32_e32 v43, v56\n"
#define RCP4 "v_rcp_f32_e32 v40, v58\n v_rcp_f32_e32 v41, v58\n v_rcp_f32_e32 v42, v58\n v_rcp_f32_e32 v43, v58\n"
// the DPP add reads the register the previous DPP add wrote: two independent VALU stand in the hazard slots, as in the row
#define DPP3 "v_fma_f32 v40, v56, s36, v40\n v_fma_f32 v41, v56, s36, v41\n" \
             "v_add_f32_dpp v59, v59, v59 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1\n"
#define FMA3 "v_fma_f32 v40, v56, s36, v40\n v_fma_f32 v41, v56, s36, v41\n v_fma_f32 v42, v56, s36, v42\n"
// a scalar ALU instruction between two VALU: does it take an issue slot from the wave?
#define VS2 "v_fma_f32 v40, v56, s36, v40\n s_add_u32 s37, s37, 0\n v_fma_f32 v41, v56, s36, v41\n s_add_u32 s37, s37, 0\n"
#define VV2 "v_fma_f32 v40, v56, s36, v40\n v_fma_f32 v41, v56, s36, v41\n"
#define SS4 "s_add_u32 s37, s37, 0\n s_add_u32 s37, s37, 0\n s_add_u32 s37, s37, 0\n s_add_u32 s37, s37, 0\n"
#define NOP4 "s_nop 0\n s_nop 0\n s_nop 0\n s_nop 0\n"
// the row fetch as the loop does it: wait for the previous request, issue the next, one row (two rows) of VALU behind it
#define ROW8 "s_waitcnt lgkmcnt(0)\n s_load_dwordx8 s[60:67], s[38:39], 0x40\n" FMA25
#define ROW16 "s_waitcnt lgkmcnt(0)\n s_load_dwordx16 s[60:75], s[38:39], 0x40\n" FMA25 FMA25
#define ROW0 FMA25
// the parts of a fetch on their own: the request without a wait inside the loop, the wait with nothing outstanding, a narrower
// request, and requests with twice the lead time
#define ROW8N "s_load_dwordx8 s[60:67], s[38:39], 0x40\n" FMA25
#define ROW16N "s_load_dwordx16 s[60:75], s[38:39], 0x40\n" FMA25 FMA25
#define ROWW "s_waitcnt lgkmcnt(0)\n" FMA25
#define ROW4 "s_waitcnt lgkmcnt(0)\n s_load_dwordx4 s[60:63], s[38:39], 0x40\n" FMA25
#define ROW8L "s_waitcnt lgkmcnt(0)\n s_load_dwordx8 s[60:67], s[38:39], 0x40\n" FMA25 FMA25
#define ROW16L "s_waitcnt lgkmcnt(0)\n s_load_dwordx16 s[60:75], s[38:39], 0x40\n" FMA25 FMA25 FMA25 FMA25
// loop control of the row loop, once per 4 rows and once per 8 rows of 25 VALU
#define CTL "s_add_u32 s38, s38, 0\n s_addc_u32 s39, s39, 0\n s_cmp_lg_u32 s38, s37\n s_cbranch_scc1 9f\n 9:\n"
#define CTL4 FMA25 FMA25 FMA25 FMA25 CTL
#define CTL8 FMA25 FMA25 FMA25 FMA25 FMA25 FMA25 FMA25 FMA25 CTL
#define ROWS4 FMA25 FMA25 FMA25 FMA25

#define STREAM(BODY) \
    asm volatile( \
        "s_mov_b32 s36, 0\n s_mov_b32 s37, 0\n s_mov_b64 s[38:39], %[p]\n s_mov_b32 s40, %[n]\n s_mov_b64 s[52:53], 0\n" \
        "v_mov_b32_e32 v56, 1.0\n v_mov_b32_e32 v57, 1.0\n v_mov_b32_e32 v58, 2.0\n v_mov_b32_e32 v59, 0\n" \
        "v_mov_b32_e32 v40, 0\n v_mov_b32_e32 v41, 0\n v_mov_b32_e32 v42, 0\n v_mov_b32_e32 v43, 0\n v_mov_b32_e32 v44, 0\n" \
        "v_mov_b32_e32 v45, 0\n v_mov_b32_e32 v46, 0\n v_mov_b32_e32 v47, 0\n v_mov_b32_e32 v48, 0\n" \
        "s_load_dwordx16 s[60:75], s[38:39], 0x0\n s_waitcnt lgkmcnt(0)\n" \
        "s_memtime %[c0]\n s_memrealtime %[r0]\n s_waitcnt lgkmcnt(0)\n" \
        "1:\n" BODY \
        "s_sub_u32 s40, s40, 1\n s_cmp_lg_u32 s40, 0\n s_cbranch_scc1 1b\n" \
        "s_waitcnt lgkmcnt(0)\n s_nop 4\n" \
        "s_memtime %[c1]\n s_memrealtime %[r1]\n s_waitcnt lgkmcnt(0)\n" \
        : [c0] "=&s"(c0), [r0] "=&s"(r0), [c1] "=&s"(c1), [r1] "=&s"(r1) \
        : [p] "s"(p), [n] "s"(n) \
        : "memory", "scc", "v40", "v41", "v42", "v43", "v44", "v45", "v46", "v47", "v48", "v56", "v57", "v58", "v59", "s36", "s37", \
          "s38", "s39", "s40", "s52", "s53", "s60", "s61", "s62", "s63", "s64", "s65", "s66", "s67", "s68", "s69", "s70", "s71", \
          "s72", "s73", "s74", "s75");

enum { T_FMA, T_PKS, T_PKO, T_EXP, T_RCP, T_DPP3, T_FMA3, T_VS, T_VV, T_SS, T_NOP, T_ROW0, T_ROW8, T_ROW16, T_ROW8N, T_ROW16N, T_ROWW, T_ROW4, T_ROW8L, T_ROW16L, T_ROWS4, T_CTL4, T_CTL8, T_COUNT };

// DOUBLE = the body twice
template <int T, bool DOUBLE>
__global__ void __launch_bounds__(64) stream(const float* p, int n, u64* out) {
    u64 c0, r0, c1, r1;
#define BODY2(B) if (DOUBLE) { STREAM(B B) } else { STREAM(B) }
    if (T == T_FMA) { BODY2(FMA8 FMA8 FMA8 FMA8) }
    else if (T == T_PKS) { BODY2(PKS4 PKS4 PKS4 PKS4 PKS4 PKS4 PKS4 PKS4) }
    else if (T == T_PKO) { BODY2(PKO4 PKO4 PKO4 PKO4 PKO4 PKO4 PKO4 PKO4) }
    else if (T == T_EXP) { BODY2(EXP4 EXP4 EXP4 EXP4 EXP4 EXP4 EXP4 EXP4) }
    else if (T == T_RCP) { BODY2(RCP4 RCP4 RCP4 RCP4 RCP4 RCP4 RCP4 RCP4) }
    else if (T == T_DPP3) { BODY2(DPP3 DPP3 DPP3 DPP3 DPP3 DPP3 DPP3 DPP3) }
    else if (T == T_FMA3) { BODY2(FMA3 FMA3 FMA3 FMA3 FMA3 FMA3 FMA3 FMA3) }
    else if (T == T_VS) { BODY2(VS2 VS2 VS2 VS2 VS2 VS2 VS2 VS2) }
    else if (T == T_VV) { BODY2(VV2 VV2 VV2 VV2 VV2 VV2 VV2 VV2) }
    else if (T == T_SS) { BODY2(SS4 SS4 SS4 SS4 SS4 SS4 SS4 SS4) }
    else if (T == T_NOP) { BODY2(NOP4 NOP4 NOP4 NOP4 NOP4 NOP4 NOP4 NOP4) }
    else if (T == T_ROW0) { BODY2(ROW0 ROW0 ROW0 ROW0) }
    else if (T == T_ROW8) { BODY2(ROW8 ROW8 ROW8 ROW8) }
    else if (T == T_ROW16) { BODY2(ROW16 ROW16) }
    else if (T == T_ROW8N) { BODY2(ROW8N ROW8N ROW8N ROW8N) }
    else if (T == T_ROW16N) { BODY2(ROW16N ROW16N) }
    else if (T == T_ROWW) { BODY2(ROWW ROWW ROWW ROWW) }
    else if (T == T_ROW4) { BODY2(ROW4 ROW4 ROW4 ROW4) }
    else if (T == T_ROW8L) { BODY2(ROW8L ROW8L) }
    else if (T == T_ROW16L) { BODY2(ROW16L) }
    else if (T == T_ROWS4) { BODY2(ROWS4 ROWS4) }
    else if (T == T_CTL4) { BODY2(CTL4 CTL4) }
    else { BODY2(CTL8) }
    if (threadIdx.x == 0) { out[0] = c1 - c0; out[1] = r1 - r0; }
}

struct Result { double cyc, ns; };

// units = instructions (or rows) in the single body
template <int T>
static Result run(const float* d, u64* d_out, int iters, int units) {
    u64 h[2][2] = {};
    for (int dbl = 0; dbl < 2; ++dbl) {
        u64 best[2] = {~0ull, ~0ull};
        for (int rep = 0; rep < 5; ++rep) {                                  // first launch warms the instruction cache
            if (dbl) hipLaunchKernelGGL((stream<T, true>), dim3(1), dim3(64), 0, 0, d, iters, d_out);
            else hipLaunchKernelGGL((stream<T, false>), dim3(1), dim3(64), 0, 0, d, iters, d_out);
            if (hipDeviceSynchronize() != hipSuccess) { fprintf(stderr, "kernel failed\n"); exit(1); }
            u64 t[2];
            (void)hipMemcpy(t, d_out, sizeof t, hipMemcpyDeviceToHost);
            if (rep > 0 && t[0] < best[0]) { best[0] = t[0]; best[1] = t[1]; }
        }
        h[dbl][0] = best[0]; h[dbl][1] = best[1];
    }
    Result r;
    r.cyc = (double)(h[1][0] - h[0][0]) / ((double)units * iters);
    r.ns = 10.0 * (double)(h[1][1] - h[0][1]) / ((double)units * iters);
    return r;
}

int main(int argc, char** argv) {
    const int iters = argc > 1 ? atoi(argv[1]) : 4000;
    float* d = nullptr;
    u64* d_out = nullptr;
    if (hipMalloc(&d, 4096) != hipSuccess || hipMalloc(&d_out, 64) != hipSuccess) return 1;
    (void)hipMemset(d, 0, 4096);
    printf("one wave alone on a CU, %d loop passes per stream; cycles from s_memtime, ns from s_memrealtime (100 MHz)\n", iters);
    printf("%-74s %8s %8s %8s\n", "stream (unit)", "cyc/unit", "ns/unit", "GHz");
#define ROW(T, units, name) { const Result r = run<T>(d, d_out, iters, units); \
        printf("%-74s %8.2f %8.3f %8.3f\n", name, r.cyc, r.ns, r.cyc / r.ns); fflush(stdout); res[T] = r; }
    Result res[T_COUNT];
    ROW(T_FMA, 32, "v_fma_f32 (instruction)")
    ROW(T_PKS, 32, "v_pk_fma_f32 v, s[pair], v, v (instruction)")
    ROW(T_PKO, 32, "v_pk_fma_f32 v, v, s[pair], v op_sel_hi:[0,1,1] (instruction)")
    ROW(T_EXP, 32, "v_exp_f32 (instruction)")
    ROW(T_RCP, 32, "v_rcp_f32 (instruction)")
    ROW(T_FMA3, 8, "3 v_fma_f32 (triple)")
    ROW(T_DPP3, 8, "2 v_fma_f32 + v_add_f32_dpp reading the previous DPP result (triple)")
    ROW(T_VV, 16, "v_fma_f32 (instruction, 16 per body)")
    ROW(T_VS, 16, "v_fma_f32 + s_add_u32 interleaved (pair)")
    ROW(T_SS, 32, "s_add_u32 back to back (instruction)")
    ROW(T_NOP, 32, "s_nop 0 back to back (instruction)")
    ROW(T_ROW0, 4, "row of 25 v_fma_f32, no fetch (row)")
    ROW(T_ROW8, 4, "s_waitcnt + s_load_dwordx8 + 25 v_fma_f32 (row)")
    ROW(T_ROW16, 4, "s_waitcnt + s_load_dwordx16 + 50 v_fma_f32 (per row, 2 rows per fetch)")
    ROW(T_ROW8N, 4, "s_load_dwordx8 + 25 v_fma_f32, no wait inside the loop (row)")
    ROW(T_ROW16N, 4, "s_load_dwordx16 + 50 v_fma_f32, no wait inside the loop (per row)")
    ROW(T_ROWW, 4, "s_waitcnt with nothing outstanding + 25 v_fma_f32 (row)")
    ROW(T_ROW4, 4, "s_waitcnt + s_load_dwordx4 + 25 v_fma_f32 (row)")
    ROW(T_ROW8L, 4, "s_waitcnt + s_load_dwordx8 + 50 v_fma_f32 (per row, 2 rows per fetch)")
    ROW(T_ROW16L, 4, "s_waitcnt + s_load_dwordx16 + 100 v_fma_f32 (per row, 4 rows per fetch)")
    ROW(T_ROWS4, 8, "4 rows of 25 v_fma_f32 (row)")
    ROW(T_CTL4, 8, "4 rows of 25 v_fma_f32 + s_add/s_addc/s_cmp/s_cbranch (row)")
    ROW(T_CTL8, 8, "8 rows of 25 v_fma_f32 + s_add/s_addc/s_cmp/s_cbranch (row)")
    printf("\nderived, cycles:\n");
    printf("  v_add_f32_dpp behind two hazard slots            %6.2f\n", res[T_DPP3].cyc - res[T_FMA3].cyc + res[T_FMA].cyc);
    printf("  s_add_u32 between two VALU                       %6.2f\n", res[T_VS].cyc - res[T_VV].cyc);
    printf("  s_waitcnt + s_load_dwordx8 per row               %6.2f\n", res[T_ROW8].cyc - res[T_ROW0].cyc);
    printf("  s_waitcnt + s_load_dwordx16 per row (of a pair)  %6.2f\n", res[T_ROW16].cyc - res[T_ROW0].cyc);
    printf("  s_load_dwordx8 alone, per request                %6.2f\n", res[T_ROW8N].cyc - res[T_ROW0].cyc);
    printf("  s_load_dwordx16 alone, per request               %6.2f\n", 2 * (res[T_ROW16N].cyc - res[T_ROW0].cyc));
    printf("  s_waitcnt with nothing outstanding               %6.2f\n", res[T_ROWW].cyc - res[T_ROW0].cyc);
    printf("  s_waitcnt + s_load_dwordx4, per request          %6.2f\n", res[T_ROW4].cyc - res[T_ROW0].cyc);
    printf("  s_waitcnt + s_load_dwordx8, 2 rows of lead       %6.2f\n", 2 * (res[T_ROW8L].cyc - res[T_ROW0].cyc));
    printf("  s_waitcnt + s_load_dwordx16, 4 rows of lead      %6.2f\n", 4 * (res[T_ROW16L].cyc - res[T_ROW0].cyc));
    printf("  loop control per row, once per 4 rows            %6.2f\n", res[T_CTL4].cyc - res[T_ROWS4].cyc);
    printf("  loop control per row, once per 8 rows            %6.2f\n", res[T_CTL8].cyc - res[T_ROWS4].cyc);
    return 0;
}
