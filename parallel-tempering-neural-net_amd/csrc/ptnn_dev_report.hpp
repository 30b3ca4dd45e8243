// ptnn_dev_report.hpp -- part of ptnn_analysis.hip (textually included there, inside namespace ptnn, after ptnn_dev_select.hpp;
// not a stand-alone header): the classification report (ptnn_class_report, include/ptnn.h).  Every kernel is
// shape-independent and reads the fx [row * K + class][u] image that AnalysisShape::predict_fwd wrote for a block of distinct samples
// (stride = the samples of the block), and the class of every row as an integer.  Per distinct sample u, exact integers:
//   1. report_labels_kernel: the class of every data row as an int (-1: not an integer in [0, K)).
//   2. report_confusion_kernel: conf[i * K + j][u] = rows of class i whose argmax over the K probabilities -- first index on a tie,
//      the rule of predict_reduce_kernel's vote -- is j.  Lanes run over u (the loads of a row's K columns coalesce), the counts
//      of a tile of samples sit in LDS as [cell][sample] (a wave's adds of one row fall into consecutive banks), and a work-group
//      adds its chunk of rows to global memory with one integer atomic per non-zero cell.
//   3. report_auc_kernel: one work-group per (sample, class k).  The N scores p[n, k] become the words pred_key(p) << 32 | [y_n == k]
//      in LDS; a bitonic sort orders them (equal keys are equal fp32 values, and inside a run of ties the negatives come first);
//      the count of negatives before every position goes into the low half of its word (one scan over the threads' chunks); a
//      positive at position s whose run of ties starts at a then adds neg(a) + neg(s) = 2 #{negatives below} + #{negatives tied}:
//      auc2[k][u] = twice the Mann-Whitney U statistic with ties counted half, an integer whatever the order of the work.
//   4. report_metrics_kernel: a thread per sample turns conf and auc2 into the Q fp32 columns img [q][u], each from exact integers
//      by one division in double (a mean over classes: the sum of those quotients in class order, divided by their count); an
//      undefined column (no row of the class, no class left) is 0, never NaN: the order-statistic select reads the image.
//   5. report_confusion_sum_kernel: one work-group per cell, sum_u cnt[u] conf[cell][u] in int64.
// predict_reduce_kernel (ptnn_dev_select.hpp) reduces img over the samples as it reduces a block of outputs.  No floating-point
// atomics.  Nothing here writes chain state, tapes, counters or trace rows.

constexpr int REPORT_THREADS = 256;            // 4 waves: every kernel but the AUC sort of many rows
constexpr int REPORT_SORT_THREADS = 1024;      // the AUC kernel above REPORT_SORT_SMALL words
constexpr int REPORT_SORT_SMALL = 2048;
constexpr int REPORT_MAX_AUC_ROWS = 16384;     // include/ptnn.h: PTNN_REPORT_MAX_AUC_ROWS; 16384 words = 128 KiB of LDS
constexpr int REPORT_CONF_LDS = 48 * 1024;     // the LDS counts of one confusion work-group stay under this

// 1. labels
__global__ void __launch_bounds__(REPORT_THREADS) report_labels_kernel(const float* y, int ys, int n_rows, int K, int* label) {
    const int n = blockIdx.x * REPORT_THREADS + threadIdx.x;
    if (n >= n_rows) return;
    const float v = y[(size_t)n * ys];
    label[n] = (v >= 0.0f && v < (float)K && v == floorf(v)) ? (int)v : -1;
}

// 2. confusion counts of a block of samples
struct ReportConf {
    const float* fx;            // [n_rows * K][stride]
    const int* label;           // [n_rows]
    int n_rows, K, stride;      // stride = samples of the block
    int TU;                     // samples per work-group, a power of two <= 64
    int rows_per_group;         // rows per blockIdx.y
    int U, u0;                  // samples of the call, the block's first
    int* conf;                  // [K * K][U], zeroed by the host
};
__global__ void __launch_bounds__(REPORT_THREADS) report_confusion_kernel(const ReportConf a) {
    extern __shared__ int cells[];                      // [K * K][TU]
    const int tid = threadIdx.x, K = a.K, KK = K * K, TU = a.TU;
    const int su = tid & (TU - 1), phase = tid / TU, phases = REPORT_THREADS / TU;
    const int ub = blockIdx.x * TU + su;                // sample within the block
    const bool live = ub < a.stride;
    for (int i = tid; i < KK * TU; i += REPORT_THREADS) cells[i] = 0;
    __syncthreads();
    const int r0 = blockIdx.y * a.rows_per_group, r1 = min(a.n_rows, r0 + a.rows_per_group);
    for (int n = r0 + phase; n < r1 && live; n += phases) {
        const int y = a.label[n];
        if (y < 0) continue;                            // refused by the host before the launch; never an index
        const float* p = a.fx + (size_t)n * K * a.stride + ub;
        int best = 0;
        float bv = p[0];
        for (int q = 1; q < K; ++q) {
            const float v = p[(size_t)q * a.stride];
            if (v > bv) { bv = v; best = q; }           // first index wins a tie (np.argmax)
        }
        atomicAdd(&cells[(y * K + best) * TU + su], 1);
    }
    __syncthreads();
    for (int i = tid; i < KK * TU; i += REPORT_THREADS) {
        const int u = blockIdx.x * TU + (i & (TU - 1));
        if (cells[i] && u < a.stride) atomicAdd(&a.conf[(size_t)(i / TU) * a.U + a.u0 + u], cells[i]);
    }
}

// 3. twice the Mann-Whitney U of every (sample, class) of a block
struct ReportAuc {
    const float* fx;            // [n_rows * K][stride]
    const int* label;           // [n_rows]
    int n_rows, K, stride;
    int npow;                   // n_rows rounded up to a power of two
    int U, u0;
    long long* auc2;            // [K][U]
};
template <int NT>
__global__ void __launch_bounds__(NT) report_auc_kernel(const ReportAuc a) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long words[];      // [npow] sort words, then [NT] scan / sum buffer
    long long* part = reinterpret_cast<long long*>(words + a.npow);
    const int tid = threadIdx.x, ub = blockIdx.x, k = blockIdx.y;
    const int N = a.n_rows, npow = a.npow;
    for (int n = tid; n < npow; n += NT) {
        unsigned long long w = ~0ull;                   // the padding sorts last
        if (n < N) {
            const float v = a.fx[((size_t)n * a.K + k) * a.stride + ub];
            w = ((unsigned long long)pred_key(v == 0.0f ? 0.0f : v) << 32) | (a.label[n] == k ? 1ull : 0ull);
        }
        words[n] = w;
    }
    __syncthreads();
    // bitonic sort, ascending: pair i of a step is (lo, lo | j), lo = i with a zero bit put in at j
    for (int size = 2; size <= npow; size <<= 1)
        for (int j = size >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < npow / 2; i += NT) {
                const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo | j;
                const unsigned long long x = words[lo], y = words[hi];
                if ((x > y) == ((lo & size) == 0)) { words[lo] = y; words[hi] = x; }
            }
            __syncthreads();
        }
    // the negatives before every position, into the low half of its word: thread tid owns positions [p0, p1)
    const int per = (npow + NT - 1) / NT;
    const int p0 = min(N, tid * per), p1 = min(N, p0 + per);
    long long c = 0;
    for (int s = p0; s < p1; ++s) c += 1 - (long long)(words[s] & 1ull);
    part[tid] = c;
    __syncthreads();
    wg_incl_scan<NT>(part, tid);
    unsigned neg = (unsigned)(part[tid] - c);
    for (int s = p0; s < p1; ++s) {
        const unsigned long long w = words[s];
        words[s] = (w & 0xffffffff00000001ull) | ((unsigned long long)neg << 1);
        neg += 1u - (unsigned)(w & 1ull);
    }
    __syncthreads();
    // a positive at s: negatives before the start of its run of ties + negatives before s (the run's negatives precede it)
    long long sum = 0;
    for (int s = tid; s < N; s += NT) {
        const unsigned long long w = words[s];
        if (!(w & 1ull)) continue;
        const unsigned key = (unsigned)(w >> 32);
        int lo = 0, hi = s;                             // the first position whose key is `key`
        if (s > 0 && (unsigned)(words[s - 1] >> 32) == key) {
            while (lo < hi) {
                const int mid = lo + ((hi - lo) >> 1);
                if ((unsigned)(words[mid] >> 32) >= key) hi = mid; else lo = mid + 1;
            }
        } else lo = s;
        sum += (long long)(((unsigned)words[lo]) >> 1) + (long long)(((unsigned)w) >> 1);
    }
    sum = wg_sum<NT>(part, sum);
    if (tid == 0) a.auc2[(size_t)k * a.U + a.u0 + ub] = sum;
}

// 4. the metric columns of every sample
struct ReportMetrics {
    const int* conf;            // [K * K][U]
    const long long* auc2;      // [K][U], or null: no auc columns
    int U, K, n_rows;
    float* img;                 // [Q][U], Q = 4 + 4 K with auc2, else 3 + 3 K
};
__global__ void __launch_bounds__(REPORT_THREADS) report_metrics_kernel(const ReportMetrics a) {
    const int u = blockIdx.x * REPORT_THREADS + threadIdx.x;
    if (u >= a.U) return;
    const int K = a.K, N = a.n_rows;
    const size_t U = (size_t)a.U;
    const bool auc = a.auc2 != nullptr;
    const int head = auc ? 4 : 3;
    float* prec = a.img + (size_t)head * U + u;
    float* rec = prec + (size_t)K * U;
    float* f1 = rec + (size_t)K * U;
    float* au = f1 + (size_t)K * U;
    long long trace = 0;
    double s_rec = 0.0, s_f1 = 0.0, s_auc = 0.0;
    int present = 0, ranked = 0;
    for (int k = 0; k < K; ++k) {
        long long nk = 0, col = 0;
        for (int j = 0; j < K; ++j) {
            nk += a.conf[(size_t)(k * K + j) * U + u];
            col += a.conf[(size_t)(j * K + k) * U + u];
        }
        const long long hit = a.conf[(size_t)(k * K + k) * U + u];
        trace += hit;
        const double p = col > 0 ? (double)hit / (double)col : 0.0;
        double r = 0.0, f = 0.0;
        if (nk > 0) {
            r = (double)hit / (double)nk;
            f = (double)(2 * hit) / (double)(nk + col);
            s_rec += r; s_f1 += f; ++present;
        }
        prec[(size_t)k * U] = (float)p;
        rec[(size_t)k * U] = (float)r;
        f1[(size_t)k * U] = (float)f;
        if (auc) {
            double v = 0.0;
            if (nk > 0 && nk < N) {
                v = (double)a.auc2[(size_t)k * U + u] / (double)(2 * nk * (N - nk));
                s_auc += v; ++ranked;
            }
            au[(size_t)k * U] = (float)v;
        }
    }
    a.img[u] = (float)((double)trace / (double)N);
    a.img[U + u] = (float)(present ? s_rec / (double)present : 0.0);
    a.img[2 * U + u] = (float)(present ? s_f1 / (double)present : 0.0);
    if (auc) a.img[3 * U + u] = (float)(ranked ? s_auc / (double)ranked : 0.0);
}

// 5. the confusion matrix summed over the expanded multiset
__global__ void __launch_bounds__(REPORT_THREADS) report_confusion_sum_kernel(const int* conf, const int* cnt, int U, long long* out) {
    __shared__ long long buf[REPORT_THREADS];
    const int* c = conf + (size_t)blockIdx.x * U;
    long long s = 0;
    for (int u = threadIdx.x; u < U; u += REPORT_THREADS) s += (long long)cnt[u] * c[u];
    s = wg_sum<REPORT_THREADS>(buf, s);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}
