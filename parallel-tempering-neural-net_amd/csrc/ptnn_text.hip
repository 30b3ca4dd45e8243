// ptnn_text.hip -- the text output of libptnn.so (ptnn_savetxt*, ptnn_text_round*, ptnn_posterior_matrix): np.savetxt's bytes
// through ptnn_text.hpp, and the posterior matrix show_results builds.  Pure host code: no HIP call, no device header.
#include "ptnn_host.hpp"
#include "ptnn_text.hpp"

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

using namespace ptnn;

extern "C" {

// exactly one floating conversion: % [flags] [width] [.precision] (e|E|f|F|g|G)
static bool float_format_ok(const char* fmt) {
    const size_t fl = std::strlen(fmt);
    bool ok = fl >= 2 && fl < 16 && fmt[0] == '%' && std::strchr("eEfFgG", fmt[fl - 1]) != nullptr;
    for (size_t k = 1; ok && k + 1 < fl; ++k) ok = std::strchr("0123456789.+- #", fmt[k]) != nullptr;
    // width and precision stay far inside the 400-byte slot ptnn_savetxt formats a value into
    for (size_t k = 1; ok && k + 1 < fl;) {
        if (fmt[k] >= '0' && fmt[k] <= '9') {
            long v = 0;
            while (k + 1 < fl && fmt[k] >= '0' && fmt[k] <= '9') v = v * 10 + (fmt[k++] - '0');
            ok = v <= 40;
        } else ++k;
    }
    return ok;
}

int ptnn_text_round(double* values, int64_t n, const char* fmt) {
    if (!values || !fmt || n < 0) return fail(-1, "bad argument");
    if (!float_format_ok(fmt)) return fail(-1, "unsupported format '%s'", fmt);
    const ptnn_text::Format f = ptnn_text::parse_format(fmt);
    for (int64_t k = 0; k < n; ++k) values[k] = ptnn_text::round_trip(values[k], f);
    return 0;
}

int ptnn_text_round_f32(const float* in, double* out, int64_t n, const char* fmt) {
    if (!in || !out || !fmt || n < 0) return fail(-1, "bad argument");
    if (!float_format_ok(fmt)) return fail(-1, "unsupported format '%s'", fmt);
    const ptnn_text::Format f = ptnn_text::parse_format(fmt);
    for (int64_t k = 0; k < n; ++k) out[k] = ptnn_text::round_trip((double)in[k], f);
    return 0;
}

}  // extern "C" (the row writer below is a template)

// rows [0, rows) of a matrix as np.savetxt writes them; value(r, c) yields the double to print, same_as_prev(r) whether row r
// repeats row r - 1 bit for bit (its text is then copied, not formatted again)
template <class Value, class SameAsPrev>
static int write_text_rows(const char* path, int64_t rows, int64_t cols, const char* fmt, bool append, Value value, SameAsPrev same_as_prev) {
    if (!float_format_ok(fmt)) return fail(-1, "unsupported format '%s'", fmt);
    const ptnn_text::Format f = ptnn_text::parse_format(fmt);
    FILE* fp = std::fopen(path, append ? "a" : "w");
    if (!fp) return fail(-4, "cannot open %s for writing", path);
    std::setvbuf(fp, nullptr, _IONBF, 0);                      // the block below is the buffer
    const size_t line_cap = (size_t)cols * 401 + 2;
    // no larger than the file can get, and not value-initialised: most of a run's files are a few KB
    const size_t buf_size = std::max<size_t>(std::min<size_t>(4u << 20, (size_t)std::max<int64_t>(rows, 1) * line_cap), 2 * line_cap);
    const std::unique_ptr<char[]> buf_mem(new char[buf_size]), line_mem(new char[line_cap]);
    struct Span { char* p; size_t n; char* data() const { return p; } size_t size() const { return n; } };
    const Span buf{buf_mem.get(), buf_size}, line{line_mem.get(), line_cap};
    size_t used = 0, line_len = 0;
    for (int64_t r = 0; r < rows; ++r) {
        if (r == 0 || !same_as_prev(r)) {
            char* o = line.data();
            for (int64_t c = 0; c < cols; ++c) {
                if (c) *o++ = ' ';
                o = ptnn_text::put_value(o, value(r, c), f);
            }
            *o++ = '\n';
            line_len = (size_t)(o - line.data());
        }
        if (buf.size() - used < line_len) {
            if (std::fwrite(buf.data(), 1, used, fp) != used) { std::fclose(fp); return fail(-4, "write to %s failed", path); }
            used = 0;
        }
        std::memcpy(buf.data() + used, line.data(), line_len);
        used += line_len;
    }
    const bool wrote = std::fwrite(buf.data(), 1, used, fp) == used;
    if (std::fclose(fp) != 0 || !wrote) return fail(-4, "write to %s failed", path);
    return 0;
}

extern "C" {

int ptnn_savetxt(const char* path, const double* data, int64_t rows, int64_t cols, const char* fmt) {
    if (!path || !data || !fmt) return fail(-1, "null argument");
    if (rows < 0 || cols < 1) return fail(-1, "bad shape %lld x %lld", (long long)rows, (long long)cols);
    return write_text_rows(path, rows, cols, fmt, false, [&](int64_t r, int64_t c) { return data[r * cols + c]; },
                           [&](int64_t r) { return std::memcmp(data + r * cols, data + (r - 1) * cols, (size_t)cols * sizeof(double)) == 0; });
}

int ptnn_savetxt_f32(const char* path, const float* data, int64_t rows, int64_t cols, int64_t row_stride, const char* fmt, int append) {
    if (!path || !data || !fmt) return fail(-1, "null argument");
    if (rows < 0 || cols < 1 || row_stride < cols) return fail(-1, "bad shape %lld x %lld (row stride %lld)", (long long)rows, (long long)cols, (long long)row_stride);
    return write_text_rows(path, rows, cols, fmt, append != 0, [&](int64_t r, int64_t c) { return (double)data[r * row_stride + c]; },
                           [&](int64_t r) { return std::memcmp(data + r * row_stride, data + (r - 1) * row_stride, (size_t)cols * sizeof(float)) == 0; });
}

int ptnn_savetxt_f32_batch(int n_files, const char* const* paths, const float* const* data, const int64_t* rows, const int64_t* cols,
                           const int64_t* row_stride, const char* const* fmts, int append, int threads) {
    if (n_files < 0 || (n_files && (!paths || !data || !rows || !cols || !row_stride || !fmts))) return fail(-1, "null argument");
    const int T = std::max(1, std::min(threads, n_files));
    std::atomic<int> next{0}, bad{-1};
    std::mutex mu;
    std::string why;
    auto work = [&]() {
        for (int k = next.fetch_add(1); k < n_files; k = next.fetch_add(1)) {
            if (ptnn_savetxt_f32(paths[k], data[k], rows[k], cols[k], row_stride[k], fmts[k], append) < 0) {
                std::lock_guard<std::mutex> lock(mu);
                if (bad.load() < 0) { bad.store(k); why = g_err; }     // g_err is per thread: carry the first cause to the caller's
            }
        }
    };
    if (T == 1) work();
    else {
        std::vector<std::thread> th;
        for (int t = 0; t < T; ++t) th.emplace_back(work);
        for (auto& x : th) x.join();
    }
    if (bad.load() >= 0) return fail(-4, "%s", why.c_str());
    return 0;
}

int ptnn_posterior_matrix(const float* pos_w, int64_t n_chains, int64_t n_rows, int64_t n_param, int64_t row_floats, int64_t first_row, double* out, int threads) {
    // out[p][c * m + t] = pos_w[c][first_row + t][p], m = n_rows - first_row: the (P, R (S - b)) float64 matrix show_results
    // returns (REG:795-797, 848: np.loadtxt of every chain's pos_w file, burn-in cut, chains side by side, transposed)
    if (!pos_w || !out || n_chains < 1 || n_param < 1 || row_floats < n_param || first_row < 0 || first_row > n_rows) return fail(-1, "bad argument");
    const int64_t m = n_rows - first_row;
    const int T = (int)std::max<int64_t>(1, std::min<int64_t>(threads, n_chains));
    auto work = [&](int t) {
        for (int64_t c = t; c < n_chains; c += T) {
            const float* src = pos_w + (c * n_rows + first_row) * row_floats;
            // blocks of rows: the block's source (bt x P floats) stays in cache while it is read P times with stride P
            for (int64_t t0 = 0; t0 < m; t0 += 256) {
                const int64_t bt = std::min<int64_t>(256, m - t0);
                for (int64_t p = 0; p < n_param; ++p) {
                    double* dst = out + p * (n_chains * m) + c * m + t0;
                    const float* s = src + t0 * row_floats + p;
                    for (int64_t k = 0; k < bt; ++k) dst[k] = (double)s[k * row_floats];
                }
            }
        }
    };
    if (T == 1) work(0);
    else {
        std::vector<std::thread> th;
        for (int t = 0; t < T; ++t) th.emplace_back(work, t);
        for (auto& x : th) x.join();
    }
    return 0;
}

}  // extern "C"
