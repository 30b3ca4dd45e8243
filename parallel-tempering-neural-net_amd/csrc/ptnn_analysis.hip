// ptnn_analysis.hip -- the 22 posterior analysis calls of libptnn.so: predict, sensitivity, partial_dependence, accumulated_effects,
// coalition_values, convergence, rank_convergence, elpd, lfo, forecast, evidence, mbar, calibration, forecast_score, ppc, powerscale,
// prior_predictive, class_report, uncertainty, influence, modes, compress, with the sample-selection path they share (SampleSource,
// distinct_samples) and their frames: RowsByVectors (input rows x weight vectors: the eight calls that read w and the eight scored
// calls that read (w, eta)), Columns and SignedColumns (summaries per column), MixtureColumns (calibration, forecast_score),
// SampleDistances (modes, compress), RungLayout and EvidEval (evidence, mbar).  The shape-independent analysis kernels are defined
// in this object: it includes them.
#include "ptnn_shapes.hpp"                   // PTNN_SHAPES
#include "ptnn_analysis_device.hpp"          // the per-shape forward kernels and their table, AnalysisShape
namespace ptnn {
#include "ptnn_dev_wg.hpp"                   // work-group reductions and scans of every kernel below (ptnn_device.hpp has included it: ladder_round)
#include "ptnn_dev_select.hpp"               // sample selection (run-length pass over the selected rows) and the per-column predictive reduction
#include "ptnn_dev_convergence.hpp"          // convergence diagnostics: split-R-hat, split-ESS over trace columns
#include "ptnn_dev_elpd.hpp"                 // predictive accuracy: lppd, WAIC, PSIS-LOO per data row
#include "ptnn_dev_lfo.hpp"                  // leave-future-out cross-validation: running sums of ll, PSIS per origin
#include "ptnn_dev_evidence.hpp"             // log evidence: per-rung statistics of the full-data log-likelihood, prior draws
#include "ptnn_dev_mbar.hpp"                 // MBAR over every rung: the free-energy fixed point, the Gram matrix of the weights, resampling
#include "ptnn_dev_calibration.hpp"          // calibration: PIT, quantiles and CRPS of the predictive mixture per data row
#include "ptnn_dev_fscore.hpp"               // forecast verification: log score per column, energy score of the path per origin
#include "ptnn_dev_ppc.hpp"                  // posterior predictive checks: replicated data and test quantities per occurrence
#include "ptnn_dev_powerscale.hpp"           // power-scaling sensitivity: components, smoothed weights, order per quantity, distances
#include "ptnn_dev_prior.hpp"                // prior predictive checks: saturation counts, statistics per drawn function and over the draws
#include "ptnn_dev_rank.hpp"                 // rank-normalised convergence: sort words, average ranks, z-scores, indicators, rank histograms
#include "ptnn_dev_sensitivity_reduce.hpp"   // input sensitivity: sign counts, row sums and their weighted means
#include "ptnn_dev_pd_reduce.hpp"            // partial dependence: row sums, ranges and the weighted means of the row means
#include "ptnn_dev_ale_reduce.hpp"           // accumulated local effects: bin sums and counts, the centred curves and surfaces
#include "ptnn_dev_report.hpp"               // classification report: confusion counts, Mann-Whitney counts and metric columns per sample
#include "ptnn_dev_uncertainty.hpp"          // predictive uncertainty: entropy per sample and its mean per row, variance per column, mean noise
#include "ptnn_dev_influence.hpp"            // case influence: column moments and the tiled FP64 cross-covariance over the samples
#include "ptnn_dev_modes.hpp"                // posterior modes: the tiled FP64 all-pairs distance of the samples' outputs, density and parents
#include "ptnn_dev_compress.hpp"             // posterior compression: mean distances, the herding walk and subset energies on that matrix
}  // namespace ptnn
#include "ptnn_host.hpp"
#include "ptnn_rank_plan.hpp"               // the blocks of ptnn_rank_convergence: host arithmetic, checked on its own

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace ptnn;

// The per-shape analysis kernels (ptnn_analysis_device.hpp; a code object per shape, ptnn_analysis_shape.hip; unknown to the handle and
// ptnn.hip) and the one lookup: *fwd = the kernel `which` of the handle's shape, allowed `lds` bytes of dynamic LDS; `what` names the call.
#define X_DECL(T, I, O) extern "C" const ptnn::AnalysisShape ptnn_ashape_##T##_##I##_##O;
PTNN_SHAPES(X_DECL)
#undef X_DECL
#define X_ENTRY(T, I, O) &ptnn_ashape_##T##_##I##_##O,
static const AnalysisShape* const g_analysis_shapes[] = {PTNN_SHAPES(X_ENTRY)};
#undef X_ENTRY
template <class K> static int analysis_shape(const ptnn_handle* h, const char* what, K AnalysisShape::*which, size_t lds, K* fwd) {
    for (const AnalysisShape* s : g_analysis_shapes)
        if (s->task == h->cfg.task && s->I == h->cfg.n_in && s->O == h->cfg.n_out)
            return raise_lds_limit(reinterpret_cast<const void*>(*fwd = s->*which), lds);
    return fail(-3, "%s: no kernel compiled for task %d with %d inputs and %d outputs", what, h->cfg.task, h->cfg.n_in, h->cfg.n_out);
}

namespace {
struct DeviceScratch {            // every buffer of one analysis call, released on every return path
    std::vector<void*> ptrs;
    ~DeviceScratch() { for (void* p : ptrs) (void)hipFree(p); }
    template <typename T> hipError_t alloc(T** p, size_t n) {
        *p = nullptr;
        if (n == 0) return hipSuccess;
        void* q = nullptr;
        const hipError_t e = hipMalloc(&q, n * sizeof(T));
        if (e == hipSuccess) { ptrs.push_back(q); *p = static_cast<T*>(q); }
        return e;
    }
    template <typename T> hipError_t upload(T** p, const T* src, size_t n, hipStream_t st) {     // alloc + copy of n host values
        const hipError_t e = alloc(p, n);
        return e != hipSuccess ? e : hipMemcpyAsync(*p, src, n * sizeof(T), hipMemcpyHostToDevice, st);
    }
};

template <typename T> hipError_t fetch(T* dst, const T* src, size_t n, hipStream_t st) {   // an output the caller asked for (non-null)
    return dst ? hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyDeviceToHost, st) : hipSuccess;
}

// One kernel launch, the arguments converted to the kernel's parameter types -> hipGetLastError(): HIP_TRY(launch(...)), so that
// a failed launch is reported where it happened
template <typename... KA, typename... A>
hipError_t launch(void (*kernel)(KA...), dim3 grid, dim3 block, size_t lds, hipStream_t st, A&&... args) {
    hipLaunchKernelGGL(kernel, grid, block, lds, st, static_cast<KA>(args)...);
    return hipGetLastError();
}

// [r0, r0 + nr) of every block of `blk` rows that covers `n` rows, ascending, given to f(r0, nr); the first non-zero return ends it
template <class F> int each_block(long long n, long long blk, F f) {
    for (long long r0 = 0; r0 < n; r0 += blk)
        if (int rc = f(r0, (int)std::min<long long>(blk, n - r0))) return rc;
    return 0;
}

void split_seed(uint64_t seed, uint32_t* lo, uint32_t* hi) {     // the two Philox key words of a spec's seed
    *lo = (uint32_t)(seed & 0xffffffffu);
    *hi = (uint32_t)(seed >> 32);
}

size_t scratch_budget(const char* var) {    // $var bytes, default 1 GiB
    const char* e = std::getenv(var);
    if (e && *e) {
        const long long v = std::atoll(e);
        if (v > 0) return (size_t)v;
    }
    return (size_t)1 << 30;
}

// the first check of every analysis call: the spec itself
template <class Spec> int check_spec(const Spec* spec, const char* name) {
    if (!spec) return fail(-1, "null argument");
    if (spec->struct_bytes != (int32_t)sizeof(Spec)) return fail(-1, "%s.struct_bytes = %d, expected %d", name, spec->struct_bytes, (int)sizeof(Spec));
    return 0;
}
// the handle of an analysis call (after the argument checks): ready, and one GPU
int check_handle(ptnn_handle* h, const char* fn) {
    if (int rc = check_ready(h)) return rc;
    if (h->comm.kind != COMM_NONE) return fail(-3, "%s serves one GPU: this handle has a communicator attached", fn);
    return 0;
}
// the device work of an analysis call starts behind everything queued; a failed run is refused here
int start_device(ptnn_handle* h) {
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    return finish_stream(h);
}

// the trace rows step0, step0 + thin, ... < step0 + nsteps of the listed local replicas (NULL = all): the residency, checkpoint
// and ring rules of ptnn_get_traces; *reps = the chains, *m = rows per chain.
int select_trace_rows(const ptnn_handle* h, const int32_t* replicas, int n_replicas, int step0, int nsteps, int thin,
                      std::vector<int32_t>* reps, int* m) {
    const int S = h->cfg.n_samples, Rl = h->cfg.n_replicas_local, cap = h->cap;
    if (step0 < 0 || nsteps < 1 || step0 + nsteps > S) return fail(-1, "trace range [%d, %d) outside [0, %d)", step0, step0 + nsteps, S);
    if (step0 + nsteps > h->cur + 1) return fail(-1, "rows up to %d requested but only %d MH steps have been queued", step0 + nsteps - 1, h->cur);
    if (step0 < h->first_row) return fail(-1, "rows below %d were produced before the checkpoint these chains were restored from", h->first_row);
    if (step0 < h->cur + 1 - cap) return fail(-1, "row %d has already been overwritten in the trace ring (capacity %d, %d steps done)", step0, cap, h->cur);
    reps->clear();
    if (replicas) {
        for (int k = 0; k < n_replicas; ++k) {
            if (replicas[k] < 0 || replicas[k] >= Rl) return fail(-1, "replica %d out of range [0, %d)", replicas[k], Rl);
            reps->push_back(replicas[k]);
        }
    } else {
        for (int r = 0; r < Rl; ++r) reps->push_back(r);
    }
    *m = (nsteps + thin - 1) / thin;
    return 0;
}

// The weight vectors an analysis call reads, from the fields every spec names alike: host vectors w [n_w][P] (with eta [n_w] and
// integer multiplicities [n_w], each optional), or the trace rows of select_trace_rows.
struct SampleSource {
    bool host;                      // host vectors (ptnn_elpd: also a host loglik); else trace rows
    const float* w;
    const float* eta;
    int64_t n_w;
    const int32_t* multiplicity;
    const int32_t* replicas;
    int n_replicas, step0, nsteps, thin;
    std::vector<int32_t> reps;      // trace: the chains
    int m = 0;                      // trace: rows per chain
    long long n_items = 0, M = 0;   // host vectors or trace rows; samples, multiplicities counted
    const int32_t* weights() const { return host ? multiplicity : nullptr; }
};
template <class Spec> SampleSource source_of(const Spec& s, bool host, const float* eta) {
    return SampleSource{host, s.w, eta, s.n_w, s.multiplicity, s.replicas, s.n_replicas, s.step0, s.nsteps, s.thin};
}
// The checks that need no handle; `unit` names a host item in the message.  `required`: the call refuses an empty trace selection
// without host items as "no source", and `third` names its other host source there, if it has one.
int check_source(const SampleSource& src, const char* unit, bool required = false, const char* third = nullptr) {
    if (required && !src.host && src.nsteps < 1)
        return third ? fail(-1, "no source: nsteps = %d trace rows, and neither host vectors w nor a host %s", src.nsteps, third)
                     : fail(-1, "no source: nsteps = %d trace rows and no host vectors w", src.nsteps);
    if (src.host) return src.n_w < 1 ? fail(-1, "n_w = %lld host %s: need at least one", (long long)src.n_w, unit) : 0;
    if (src.thin < 1) return fail(-1, "thin = %d must be >= 1", src.thin);
    if (src.replicas && src.n_replicas < 1) return fail(-1, "n_replicas = %d with a replica list", src.n_replicas);
    return 0;
}
// n_items and M: host multiplicities summed (no handle needed), or the trace rows selected
int count_samples(const ptnn_handle* h, SampleSource& src) {
    if (src.host) {
        src.n_items = src.n_w;
        src.M = src.multiplicity ? 0 : src.n_w;
        for (int64_t k = 0; src.multiplicity && k < src.n_w; ++k) {
            if (src.multiplicity[k] < 0) return fail(-1, "multiplicity[%lld] = %d is negative", (long long)k, src.multiplicity[k]);
            src.M += src.multiplicity[k];
        }
        return 0;
    }
    if (int rc = select_trace_rows(h, src.replicas, src.n_replicas, src.step0, src.nsteps, src.thin, &src.reps, &src.m)) return rc;
    src.n_items = src.M = (long long)src.reps.size() * src.m;
    return 0;
}
// Before the handle: the host items of the calls whose host faults precede the handle's; their trace rows are counted in
// select_samples (host_counted)
int count_host_samples(SampleSource& src) { return src.host ? count_samples(nullptr, src) : 0; }
// After the handle: the samples counted -- `host_counted`: the host items already were, before the handle -- at least one, or two
// where `needs_two` says what for, and within the kernels' int indices
int select_samples(const ptnn_handle* h, SampleSource& src, bool host_counted, const char* needs_two = nullptr) {
    if (!(src.host && host_counted))
        if (int rc = count_samples(h, src)) return rc;
    if (needs_two && src.M < 2) return fail(-1, "the selection holds %lld samples: %s", src.M, needs_two);
    if (src.M < 1) return fail(-1, "the selection holds no sample");
    if (src.M > 0x7fffffffLL || src.n_items > 0x7fffffffLL) return fail(-1, "%lld samples: at most 2^31 - 1 per call", src.M);
    return 0;
}
// a regression's likelihood reads tau^2: host vectors come with their eta
int need_eta(const ptnn_handle* h, const SampleSource& src) {
    if (src.w && !src.eta && h->cfg.task == PTNN_TASK_REG) return fail(-1, "a regression's host vectors need eta = log tau^2 (one per vector)");
    return 0;
}

// PSIS: the relative efficiency of the draws, and the tail length of S of them
int check_r_eff(double r_eff) {
    if (!(r_eff > 0.0) || !std::isfinite(r_eff)) return fail(-1, "r_eff = %g must be a finite number > 0", r_eff);
    return 0;
}
int psis_tail(long long S, double r_eff, long long* M) {
    *M = (long long)std::ceil(std::min(0.2 * (double)S, 3.0 * std::sqrt((double)S / r_eff)));
    if (*M > ELPD_TAIL_CAP)
        return fail(-1, "%lld samples with r_eff = %g need a PSIS tail of M = %lld > %d samples: select fewer samples (thin=, chains=) "
                        "or give a larger r_eff", S, r_eff, *M, ELPD_TAIL_CAP);
    return 0;
}

// Stage a: the items of a source collapse into distinct samples -- maximal runs of bitwise-equal consecutive vectors of one chain
// or of the host list -- with integer multiplicities (sample_runs_kernel, predict_scan_kernel).  `eta`: the samples are (w, eta)
// -- a regression's eta is read, compared and checked, a classification's is 0 -- and every run gets its eta
// (elpd_run_eta_kernel).  Without `merge` every item is a sample of its own with count 1 (forecast with noise: every occurrence
// is its own trajectory).
struct Distinct {
    const float* base = nullptr;    // the vectors: d_pos_w rows or the uploaded host vectors
    long long* run_off = nullptr;   // [U] float offset of sample u in base
    int* run_cnt = nullptr;         // [U] its multiplicity
    int* item_run = nullptr;        // [n_items] the sample of every item (merge)
    float* run_eta = nullptr;       // [U] its eta (eta)
    int U = 0;
};
int distinct_samples(ptnn_handle* h, DeviceScratch& mem, const SampleSource& src, bool eta, bool merge, Distinct* d) {
    const long long n = src.n_items;
    const bool reg = eta && h->cfg.task == PTNN_TASK_REG;
    hipStream_t st = h->stream;
    long long* item_off = nullptr;
    int *flag = nullptr, *err = nullptr, *weight = nullptr, *reps = nullptr;
    float *item_eta = nullptr, *w = nullptr, *host_eta = nullptr;
    HIP_TRY(mem.alloc(&item_off, (size_t)n));
    HIP_TRY(mem.alloc(&flag, (size_t)n));
    HIP_TRY(mem.alloc(&d->run_cnt, (size_t)n));
    HIP_TRY(mem.alloc(&err, 4));        // [0] runs, [1] unresolved compact rows, [2] rows without eta, [3] the first such chain
    if (eta) HIP_TRY(mem.alloc(&item_eta, (size_t)n));
    if (merge) {
        HIP_TRY(mem.alloc(&d->run_off, (size_t)n));
        HIP_TRY(mem.alloc(&d->item_run, (size_t)n));
        if (eta) HIP_TRY(mem.alloc(&d->run_eta, (size_t)n));
        HIP_TRY(hipMemsetAsync(d->run_cnt, 0, (size_t)n * sizeof(int), st));
    } else {
        d->run_off = item_off;
        d->run_eta = item_eta;
        HIP_TRY(hipMemsetD32Async(d->run_cnt, 1, (size_t)n, st));
    }
    HIP_TRY(hipMemsetAsync(err, 0, 3 * sizeof(int), st));
    if (eta) HIP_TRY(hipMemsetAsync(err + 3, 0x7f, sizeof(int), st));
    SampleSel sel{};
    sel.reg = reg ? 1 : 0; sel.P = h->P; sel.n_items = n; sel.item_off = item_off; sel.item_eta = item_eta; sel.flag = flag;
    sel.error = err + 1;
    if (src.host) {
        HIP_TRY(mem.upload(&w, src.w, (size_t)n * h->P, st));
        if (reg) HIP_TRY(mem.upload(&host_eta, src.eta, (size_t)n, st));
        if (merge && src.multiplicity) HIP_TRY(mem.upload(&weight, src.multiplicity, (size_t)n, st));
        sel.host = 1; sel.pos_w = w; sel.host_eta = host_eta;
    } else {
        HIP_TRY(mem.upload(&reps, src.reps.data(), src.reps.size(), st));
        sel.host = 0; sel.pos_w = h->d_pos_w; sel.scal = h->d_scal; sel.replicas = reps; sel.st_i = h->d_st_i; sel.cap = h->cap;
        sel.PW = h->PW; sel.step0 = src.step0; sel.thin = src.thin; sel.m = src.m; sel.compact = h->plan.compact ? 1 : 0; sel.cur = h->cur;
    }
    d->base = sel.pos_w;
    const unsigned item_blocks = (unsigned)((n + PRED_THREADS - 1) / PRED_THREADS);
    HIP_TRY(launch(sample_runs_kernel, dim3(item_blocks), dim3(PRED_THREADS), 0, st, sel));
    if (merge) {
        PredictScan sc{n, flag, item_off, weight, d->item_run, d->run_off, d->run_cnt, err};
        HIP_TRY(launch(predict_scan_kernel, dim3(1), dim3(PRED_SCAN_THREADS), 0, st, sc));
        if (eta) HIP_TRY(launch(elpd_run_eta_kernel, dim3(item_blocks), dim3(ELPD_THREADS), 0, st, n, flag, d->item_run, item_eta, d->run_eta));
    }
    int e[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(e, err, sizeof e, hipMemcpyDeviceToHost, st));
    if (int rc = wait_stream(h)) return rc;          // also keeps the host arrays of `src` alive until the copies are done
    if (e[1]) return fail(-2, "%d selected compact trace rows refer to rows that are not resident (internal error)", e[1]);
    if (e[2]) {
        const int c = e[3] >= 0 && e[3] < (int)src.reps.size() ? e[3] : 0;
        return fail(-1, "%s%d selected trace rows precede their chain's first accepted MH step (chain %d, local replica %d, among "
                        "others): no eta = log tau^2 was recorded for them; start the selection later (a larger burn_in)",
                    merge ? "" : "noise: ", e[2], c, src.reps.empty() ? 0 : src.reps[(size_t)c]);
    }
    d->U = merge ? e[0] : (int)n;
    if (d->U < 1 || d->U > n) return fail(-2, "run-length pass found %d distinct samples among %lld rows (internal error)", d->U, n);
    return 0;
}
// the sample of every item on the host, for the selection-order outputs (queued: valid after the next wait_stream)
int item_runs(ptnn_handle* h, const Distinct& d, long long n_items, std::vector<int>* out) {
    out->resize((size_t)n_items);
    if (!d.item_run) {
        for (long long i = 0; i < n_items; ++i) (*out)[(size_t)i] = (int)i;
        return 0;
    }
    HIP_TRY(hipMemcpyAsync(out->data(), d.item_run, (size_t)n_items * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    return 0;
}
// A block of per-sample outputs blk [ncols][U] on the device, expanded to the selection's order (chain-major, item i `mult[i]`
// times, null: once): selected sample `row` gets its columns at out + row * row_stride + col0.
template <typename T>
int scatter_samples(ptnn_handle* h, const T* blk, int ncols, int U, const std::vector<int>& item_run, const int32_t* mult, T* out,
                    size_t row_stride, size_t col0) {
    std::vector<T> hb((size_t)ncols * U);
    HIP_TRY(hipMemcpyAsync(hb.data(), blk, hb.size() * sizeof(T), hipMemcpyDeviceToHost, h->stream));
    if (int rc = wait_stream(h)) return rc;
    size_t row = 0;
    for (size_t i = 0; i < item_run.size(); ++i) {
        const size_t u = (size_t)item_run[i];
        for (int k = 0, reps = mult ? mult[i] : 1; k < reps; ++k, ++row) {
            T* dst = out + row * row_stride + col0;
            for (int c = 0; c < ncols; ++c) dst[c] = hb[(size_t)c * U + u];
        }
    }
    return 0;
}

// Input rows of an analysis call: `source` PTNN_PREDICT_X_HOST with host rows, or the handle's train / test set
static_assert(PTNN_FORECAST_ORIGIN_HOST == PTNN_PREDICT_X_HOST && PTNN_FORECAST_ORIGIN_TRAIN == PTNN_PREDICT_X_TRAIN &&
              PTNN_FORECAST_ORIGIN_TEST == PTNN_PREDICT_X_TEST, "ptnn.h row sources");
struct RowSource {
    int source;
    const float* host;
    int n;
    const char *field, *prefix, *arg, *count;   // names in the messages: "x_source", "PTNN_PREDICT_X", "x", "n_rows"
};
template <class Spec> RowSource x_rows(const Spec& s) {     // the rows most specs name alike
    return RowSource{s.x_source, s.x, s.n_rows, "x_source", "PTNN_PREDICT_X", "x", "n_rows"};
}
int check_rows(const RowSource& r) {        // no handle needed
    if (r.source != PTNN_PREDICT_X_HOST && r.source != PTNN_PREDICT_X_TRAIN && r.source != PTNN_PREDICT_X_TEST)
        return fail(-1, "%s = %d is not %s_HOST, _TRAIN or _TEST", r.field, r.source, r.prefix);
    if (r.source == PTNN_PREDICT_X_HOST && !r.host) return fail(-1, "%s %s_HOST needs %s", r.field, r.prefix, r.arg);
    return 0;
}
int fit_rows(const ptnn_handle* h, const RowSource& r) {
    if (r.source == PTNN_PREDICT_X_TRAIN && r.n != h->Ntr) return fail(-1, "%s = %d but the train set has %d rows", r.count, r.n, h->Ntr);
    if (r.source == PTNN_PREDICT_X_TEST && r.n != h->Nte) return fail(-1, "%s = %d but the test set has %d rows", r.count, r.n, h->Nte);
    return 0;
}
// host rows x [n][I + 1] of a classification: the last column is a class, as ptnn_set_data checks the handle's own rows
int check_labels(const float* x, int n_rows, int I, int O) {
    for (int n = 0; n < n_rows; ++n) {
        const float yv = x[(size_t)n * (I + 1) + I];
        if (!(yv >= 0.0f) || yv >= (float)O || yv != std::floor(yv))
            return fail(-1, "class label %g in row %d is not an integer in [0, %d)", (double)yv, n, O);
    }
    return 0;
}
// the rows on the device: the host rows (`width` floats each) uploaded, or the data set; row k at *x + k * *xs
int upload_rows(ptnn_handle* h, DeviceScratch& mem, const RowSource& r, int width, const float** x, int* xs) {
    if (r.source == PTNN_PREDICT_X_HOST) {
        float* d = nullptr;
        HIP_TRY(mem.upload(&d, r.host, (size_t)r.n * width, h->stream));
        *x = d; *xs = width;
    } else {
        *x = h->d_data + (r.source == PTNN_PREDICT_X_TEST ? (size_t)h->Ntr * h->IPY : 0);
        *xs = h->IPY;
    }
    return 0;
}

// Stage b of every call whose per-shape forward kernel stages distinct vectors in LDS (Fwd = PredictFwd, SensFwd, PdFwd, AleFwd,
// ShapFwd; ptnn_dev_net.hpp): what the five plans share.  A plan's own init() is its budget arithmetic -- vectors(), then fit().
template <class Fwd> struct StagedPlan {
    int PV = 0, NV = 0, VS = 0;
    size_t lds = 0;
    void (*fwd)(const Fwd) = nullptr;
    // NV: as many vectors as `budget` floats of LDS hold at PV + `beside` floats each, at most max_nv
    void vectors(const ptnn_handle* h, int max_nv, int budget, int beside) {
        PV = round_up4(h->P);
        NV = std::max(1, std::min(max_nv, budget / (PV + beside)));
    }
    // The LDS request: per vector PV floats and its finished tile of `tile` floats (none: 0) with the pad that lands the vectors of
    // one column in different LDS banks, and `once` floats per work-group; the refusal in `what`'s name; the kernel of the shape.
    int fit(const ptnn_handle* h, const char* what, void (*AnalysisShape::*which)(const Fwd), int tile, size_t once = 0) {
        VS = tile ? tile + std::max(1, WAVE / NV) : 0;
        lds = ((size_t)NV * (PV + VS) + once) * sizeof(float);
        if (lds > LDS_CEILING) return fail(-3, "%s: a %d-parameter vector does not fit in LDS", what, h->P);
        return analysis_shape(h, what, which, lds, &fwd);
    }
    FwdCommon common(const ptnn_handle* h, const float* base, const long long* run_off, const float* x, int xs, int r0, int nr, int U) const {
        return FwdCommon{base, run_off, x, xs, r0, nr, h->cfg.n_hidden, h->P, PV, U, NV};
    }
    // groups of NV vectors x groups of `rows` rows (x nz)
    int launch_groups(const ptnn_handle* h, const Fwd& fa, int threads, int rows = WAVE, int nz = 1) const {
        HIP_TRY(launch(fwd, dim3((unsigned)((fa.c.U + NV - 1) / NV), (unsigned)((fa.c.nrows + rows - 1) / rows), (unsigned)nz),
                       dim3(threads), lds, h->stream, fa));
        return 0;
    }
};

// predict, elpd, evidence, ...: the per-shape predict_fwd.  48 KiB of LDS; beside a staged vector the four waves' partial sums and
// the transposed tile, which need no pad
struct ForwardPlan : StagedPlan<PredictFwd> {
    int init(const ptnn_handle* h, const char* what) {
        const int beside = (PRED_THREADS / WAVE + 1) * h->cfg.n_out * WAVE;
        vectors(h, PRED_MAX_NV, 48 * 1024 / 4, beside);
        return fit(h, what, &AnalysisShape::predict_fwd, 0, (size_t)NV * beside);
    }
    // fx [nr * O][U] = the outputs of vectors base + run_off[u] on rows [r0, r0 + nr) of x
    int run(const ptnn_handle* h, const float* base, const long long* run_off, const float* x, int xs, int r0, int nr, int U, float* fx) const {
        return launch_groups(h, PredictFwd{common(h, base, run_off, x, xs, r0, nr, U), fx}, PRED_THREADS);
    }
};
// rows per block of the forward pass: `budget` bytes of scratch at `row_bytes` per row, and at most 65535 work-groups of WAVE
// rows (grid.y of predict_fwd)
long long row_block(size_t budget, size_t row_bytes, long long n_rows) {
    return std::max(1LL, std::min<long long>({(long long)(budget / row_bytes), 65535LL * WAVE, n_rows}));
}

// Stage b of sensitivity: the per-shape sens_fwd, NV distinct vectors staged in LDS per work-group beside their finished 64-row
// gradient tiles (n_out * n_in * 64 floats each): as many vectors as 64 KiB hold, so that two work-groups share a CU
struct SensPlan : StagedPlan<SensFwd> {
    int init(const ptnn_handle* h) {
        const int tile = h->cfg.n_out * h->cfg.n_in * WAVE;
        vectors(h, SENS_MAX_NV, 64 * 1024 / 4, tile + WAVE);
        return fit(h, "input sensitivity", &AnalysisShape::sens_fwd, tile);
    }
    // gx [nr * O * I][U] = the input gradients of vectors base + run_off[u] on rows [r0, r0 + nr) of x
    int run(const ptnn_handle* h, const float* base, const long long* run_off, const float* x, int xs, int r0, int nr, int U, float* gx) const {
        return launch_groups(h, SensFwd{common(h, base, run_off, x, xs, r0, nr, U), VS, gx}, SENS_THREADS);
    }
};

// Stage b of partial dependence: the per-shape pd_fwd.  A work-group stages NV distinct vectors in LDS beside their finished tiles
// of one chunk: GC grid values of one selected input, n_out * GC * 64 floats each.  With GT = pd_grid_tile(n_out) grid values
// per pass, a chunk starts as the whole tiles that PD_ACC columns hold (n_out = 1: 2 x 16 values, else one tile), cut to the grid,
// so that a vector's tile stays near 10 KiB; NV = as many vectors as 64 KiB hold (two work-groups share a CU), at most 16.  Where
// that leaves fewer than four (vector, tile) pairs for the four waves -- a vector above 16 KiB -- the chunk grows tile by tile
// while the grid has more and the request stays under LDS_CEILING.  The largest compiled request is 34-512-2 with 64 grid values:
// one vector of 18948 floats and a 64-value chunk, 108 816 B.
struct PdPlan : StagedPlan<PdFwd> {
    int GC = 0, NCH = 0, A = 0, G = 0;
    int init(const ptnn_handle* h, int n_inputs, int n_grid) {
        const int O = h->cfg.n_out, GT = pd_grid_tile(O), tiles = (n_grid + GT - 1) / GT;
        A = n_inputs; G = n_grid;
        int ct = std::min(tiles, std::max(1, PD_ACC / (O * GT)));
        const auto tile = [&](int t) { return std::min(t * GT, G) * O * WAVE; };
        vectors(h, PD_MAX_NV, 64 * 1024 / 4, tile(ct) + WAVE);
        while (NV * ct < PD_THREADS / WAVE && ct < tiles && (size_t)NV * (PV + tile(ct + 1) + WAVE) * sizeof(float) <= LDS_CEILING) ++ct;
        GC = std::min(ct * GT, G);
        NCH = (G + GC - 1) / GC;
        return fit(h, "partial dependence", &AnalysisShape::pd_fwd, tile(ct));
    }
    // fx [nr * A * G * O][U] = the outputs of vectors base + run_off[u] on rows [r0, r0 + nr) of x, input inputs[a] set to grid[a, k]
    int run(const ptnn_handle* h, const float* base, const long long* run_off, const float* x, int xs, int r0, int nr, int U,
            const int* inputs, const float* grid, float* fx) const {
        return launch_groups(h, PdFwd{common(h, base, run_off, x, xs, r0, nr, U), VS, A, G, GC, NCH, inputs, grid, fx}, PD_THREADS, WAVE, A * NCH);
    }
};

// Stage b of forecast and forecast_score: the per-shape forecast_fwd.  The layout is a function of the shape alone (P), never of the
// scratch budget: FC_LANE (a lane per trajectory, 4 x 64 vectors transposed in LDS) while a vector is short enough, else FC_SPLIT.
struct ForecastPlan {
    size_t lds = 0;
    void (*fwd)(const ForecastFwd) = nullptr;
    ForecastFwd fa{};
    // what every block shares: the trajectories d from the origins x, the carried windows, the noise and its seed, the outputs
    int init(const ptnn_handle* h, const Distinct& d, const float* x, int xs, int horizon, float* win, bool noise, uint64_t seed, float* fx, float* mu) {
        const int P = h->P;
        fa.base = d.base; fa.run_off = d.run_off; fa.eta = d.run_eta; fa.x = x; fa.xs = xs; fa.horizon = horizon; fa.win = win;
        fa.H = h->cfg.n_hidden; fa.P = P; fa.U = d.U; fa.noise = noise ? 1 : 0; fa.fx = fx; fa.mu = mu;
        split_seed(seed, &fa.seed_lo, &fa.seed_hi);
        fa.layout = P <= FC_LANE_MAX_P ? FC_LANE : FC_SPLIT;
        lds = fa.layout == FC_LANE ? (size_t)(FC_THREADS / WAVE) * P * WAVE * sizeof(float)
                                   : (size_t)(round_up4(P) + 2 * (FC_THREADS / WAVE) * WAVE) * sizeof(float);
        if (lds > LDS_CEILING) return fail(-3, "forecast: a %d-parameter vector does not fit in LDS", P);
        return analysis_shape(h, "forecast", &AnalysisShape::forecast_fwd, lds, &fwd);
    }
    // fx [nr * nk][U] (and mu) = steps [k0, k0 + nk) of the trajectories from origins [r0, r0 + nr)
    int run(const ptnn_handle* h, int r0, int nr, int k0, int nk) {
        fa.r0 = r0; fa.nr = nr; fa.k0 = k0; fa.hb = nk;
        const long long gx = (fa.U + FC_THREADS - 1) / FC_THREADS;      // FC_LANE
        const dim3 grid = fa.layout == FC_LANE ? dim3((unsigned)gx, (unsigned)std::max(1LL, std::min<long long>((512 + gx - 1) / gx, nr)))
                                               : dim3((unsigned)fa.U, (unsigned)((nr + WAVE - 1) / WAVE));
        HIP_TRY(launch(fwd, grid, dim3(FC_THREADS), lds, h->stream, fa));
        return 0;
    }
};
// forecasts with noise: every occurrence is its own trajectory, so host multiplicities are expanded into w_exp / eta_exp, which
// `src` then names
void expand_occurrences(SampleSource& src, int P, std::vector<float>* w_exp, std::vector<float>* eta_exp) {
    if (!src.host || !src.multiplicity) return;
    w_exp->reserve((size_t)src.M * P); eta_exp->reserve((size_t)src.M);
    for (int64_t k = 0; k < src.n_w; ++k)
        for (int c = 0; c < src.multiplicity[k]; ++c) {
            w_exp->insert(w_exp->end(), src.w + (size_t)k * P, src.w + (size_t)(k + 1) * P);
            eta_exp->push_back(src.eta[k]);
        }
    src.w = w_exp->data(); src.eta = eta_exp->data(); src.multiplicity = nullptr; src.n_items = src.M;
}

// The order statistics of predict, sensitivity and forecast: ranks [n] in the expanded multiset of M samples, the values of those
// ranks in every column to the caller's order_stats
struct RankOutputs {
    int n;
    const int64_t* ranks;
    const void* order_stats;
    long long* d_ranks = nullptr;
    float* d_stats = nullptr;           // [n][ncols]
    int check() const {                 // no handle needed
        if (n < 0 || n > PTNN_PREDICT_MAX_RANKS) return fail(-1, "n_ranks = %d outside [0, %d]", n, PTNN_PREDICT_MAX_RANKS);
        if (n > 0 && !ranks) return fail(-1, "n_ranks = %d but ranks is NULL", n);
        if (order_stats && n == 0) return fail(-1, "order_stats requested without ranks");
        return 0;
    }
    int check_values(long long M) const {
        for (int k = 0; k < n; ++k)
            if (ranks[k] < 0 || ranks[k] >= M) return fail(-1, "rank %lld outside [0, %lld)", (long long)ranks[k], M);
        return 0;
    }
    int to_device(DeviceScratch& mem, size_t ncols, hipStream_t st) {
        if (n == 0) return 0;
        HIP_TRY(mem.alloc(&d_stats, (size_t)n * ncols));
        HIP_TRY(mem.upload(&d_ranks, (const long long*)ranks, (size_t)n, st));
        return 0;
    }
};

// the counts of n host samples that are each their own entry, on the device: their multiplicities, or ones
int upload_counts(ptnn_handle* h, DeviceScratch& mem, const int32_t* multiplicity, size_t n, int** d_cnt) {
    std::vector<int32_t> ones(multiplicity ? 0 : n, 1);
    HIP_TRY(mem.upload(d_cnt, multiplicity ? multiplicity : ones.data(), n, h->stream));
    return multiplicity ? 0 : wait_stream(h);            // `ones` dies at the end of this function
}
// the host loglik on the device: every host sample is its own entry of `ra` (repeats need no merging: the reductions depend on the
// multiset only)
template <class Spec> int upload_loglik(ptnn_handle* h, DeviceScratch& mem, const Spec& s, long long n_items, ElpdRed* ra) {
    double* d_ll = nullptr;
    int* d_cnt = nullptr;
    HIP_TRY(mem.upload(&d_ll, s.loglik, (size_t)n_items * s.n_rows, h->stream));
    if (int rc = upload_counts(h, mem, s.multiplicity, (size_t)n_items, &d_cnt)) return rc;
    ra->mode = ELPD_HOST; ra->ll = d_ll; ra->ll_stride = s.n_rows; ra->cnt = d_cnt; ra->U = (int)n_items;
    return 0;
}
// elpd_loglik_kernel on the block of `nr` rows that `ra` names -> ra.ll_out [nr][U]
int loglik_block(ptnn_handle* h, const ElpdRed& ra, int nr) {
    const long long n_ll = (long long)nr * ra.U;
    HIP_TRY(launch(elpd_loglik_kernel, dim3((unsigned)((n_ll + ELPD_THREADS - 1) / ELPD_THREADS)), dim3(ELPD_THREADS), 0, h->stream, ra, nr));
    return 0;
}

// The log-likelihood of the rows [r0, r0 + nr) of x (the target behind the n_in inputs) on every distinct sample, as ptnn_elpd forms
// it -> dst [nr][U]: the forward pass into fx, then elpd_loglik_kernel; the caller's `ra` names the task, eta and the counts
int loglik_rows(ptnn_handle* h, const ForwardPlan& fwd, const Distinct& d, const float* x, int xs, long long r0, int nr, float* fx,
                double* dst, ElpdRed ra) {
    if (int rc = fwd.run(h, d.base, d.run_off, x, xs, (int)r0, nr, ra.U, fx)) return rc;
    ra.fx = fx; ra.y = x + h->cfg.n_in; ra.ys = xs; ra.row0 = (int)r0; ra.ll_out = dst;
    return loglik_block(h, ra, nr);
}

// The frame of the calls that take input rows x and weight vectors w, in three steps, since the order of the refusals is kept and
// every call has checks of its own between them: the checks before the handle, the samples selected with the handle, the rows and
// the distinct samples on the device.  Two kinds of call stand on it.  predict, sensitivity, partial_dependence,
// accumulated_effects, coalition_values, class_report, modes and compress read vectors w: check(), select(), stage().  The scored
// calls -- elpd, lfo, calibration, forecast_score, ppc, powerscale, uncertainty, influence -- read samples (w, eta) and mostly a
// target column behind the inputs: their host items are counted before the handle, so they name the parts of check() one by one
// (check_source(), ::check_rows(rows), count_host()) around their own checks, then fit(), select() and stage() alike.
struct RowsByVectors {
    SampleSource src;
    RowSource rows;
    RankOutputs rk, rk2;                    // rk2: the ranks of a second quantity, for the calls that have one
    const bool scored = false;              // a scored call: (w, eta) samples, the host items counted before the handle
    bool eta = false, merge = true;         // stage: distinct_samples' flags; a scored call sets them first
    bool started = false;
    long long M = 0;                        // select: the samples, multiplicities counted
    DeviceScratch mem;                      // stage: every buffer of the call
    const float* d_x = nullptr;             // stage: row k at d_x + k * xs
    int xs = 0, U = 0;
    Distinct d;
    std::vector<int> item_run;              // items: the sample of every item, for the selection-order outputs
    ForwardPlan fwd;                        // forward: the forward pass and its scratch d_fx [rows_blk * O][U]
    long long rows_blk = 0;
    float* d_fx = nullptr;
    template <class Spec> RowsByVectors(const Spec& s, RankOutputs rk, RankOutputs rk2 = RankOutputs{0, nullptr, nullptr})
        : src(source_of(s, s.w != nullptr, nullptr)), rows(x_rows(s)), rk(rk), rk2(rk2) {}
    // a scored call; `host`: host items -- vectors w, or the call's third source
    template <class Spec> RowsByVectors(const Spec& s, const RowSource& rows, bool host, RankOutputs rk = RankOutputs{0, nullptr, nullptr})
        : src(source_of(s, host, s.eta)), rows(rows), rk(rk), rk2{0, nullptr, nullptr}, scored(true) {}
    // no handle needed; `one_grid`: the rows are one dimension of a grid of WAVE-row work-groups
    int check(bool one_grid = false) const {
        if (int rc = ::check_source(src, "vectors")) return rc;
        if (int rc = check_rows(rows)) return rc;
        if (rows.n < 1) return fail(-1, "n_rows = %d must be >= 1", rows.n);
        if (one_grid && rows.n > 65535 * WAVE) return fail(-1, "n_rows = %d: at most 65535 x 64 rows per call", rows.n);
        if (int rc = rk.check()) return rc;
        return rk2.check();
    }
    int check_source(const char* third = nullptr) const { return ::check_source(src, "samples", true, third); }
    int count_host() { return count_host_samples(src); }
    // with the handle: a regression's host vectors bring eta, the rows are the data set's
    int fit(const ptnn_handle* h, bool with_rows = true) const {
        if (int rc = need_eta(h, src)) return rc;
        return with_rows ? fit_rows(h, rows) : 0;
    }
    int select(const ptnn_handle* h, int64_t* n_samples, const char* needs_two = nullptr) {
        if (int rc = select_samples(h, src, scored, needs_two)) return rc;
        M = src.M;
        if (int rc = rk.check_values(M)) return rc;
        if (int rc = rk2.check_values(M)) return rc;
        if (n_samples) *n_samples = M;
        return 0;
    }
    // the device work starts once: stage() starts it, or a call with buffers or a source of its own before the rows
    int start(ptnn_handle* h) { return started ? 0 : (started = true, start_device(h)); }
    // rows of `width` floats (0: none); `uploads` queues the call's own tables between the rows and the run-length pass
    template <class F> int stage(ptnn_handle* h, int width, int64_t* n_distinct, F uploads) {
        if (int rc = start(h)) return rc;
        if (width)
            if (int rc = upload_rows(h, mem, rows, width, &d_x, &xs)) return rc;
        if (int rc = uploads()) return rc;
        if (int rc = distinct_samples(h, mem, src, eta, merge, &d)) return rc;
        U = d.U;
        if (n_distinct) *n_distinct = U;
        return 0;
    }
    int stage(ptnn_handle* h, int width, int64_t* n_distinct) { return stage(h, width, n_distinct, [] { return 0; }); }
    int items(ptnn_handle* h, bool wanted) { return wanted ? item_runs(h, d, src.n_items, &item_run) : 0; }
    // The forward scratch: blocks of the `n` rows under $budget_var -- `part` of it, at `row_bytes` per row, the fp32 outputs and
    // what the call keeps beside them -- and the plan; `what` names the call
    int forward(ptnn_handle* h, const char* budget_var, size_t part, size_t row_bytes, long long n, const char* what) {
        rows_blk = row_block(scratch_budget(budget_var) / part, row_bytes, n);
        HIP_TRY(mem.alloc(&d_fx, (size_t)rows_blk * h->cfg.n_out * U));
        return fwd.init(h, what);
    }
    // the blocks of rows [0, n), ascending: the forward pass of [r0, r0 + nr) into d_fx, then body(r0, nr)
    template <class F> int each_rows(ptnn_handle* h, long long n, F body) {
        return each_block(n, rows_blk, [&](long long r0, int nr) -> int {
            if (int rc = fwd.run(h, d.base, d.run_off, d_x, xs, (int)r0, nr, U, d_fx)) return rc;
            return body(r0, nr);
        });
    }
};

// The pointwise log-likelihood of ptnn_elpd and ptnn_lfo (one Spec's fields are the other's): the frame's sources -- trace rows or
// host vectors (w, eta) -- or a host loglik [n_w][n_rows], a branch of the two calls' own.  The argument checks they share, in three
// parts, since the order of the refusals is kept and ptnn_lfo has checks of its own between them.
template <class Spec> int pointwise_source(const Spec& s, const RowsByVectors& f) {
    if (s.loglik && s.w) return fail(-1, "give host vectors w or a host loglik, not both");
    if (int rc = check_r_eff(s.r_eff)) return rc;
    if (int rc = f.check_source("loglik")) return rc;
    if (s.n_rows < 1) return fail(-1, "n_rows = %d must be >= 1", s.n_rows);
    return 0;
}
template <class Spec> int pointwise_rows(const Spec& s, RowsByVectors& f) {   // ends with the host samples counted
    if (!s.loglik)
        if (int rc = check_rows(f.rows)) return rc;
    if (s.loglik && s.loglik_out) return fail(-1, "loglik_out: the log-likelihood is the input of this source");
    if (int rc = f.count_host()) return rc;
    if (s.loglik)
        for (long long k = 0; k < f.src.n_items * s.n_rows; ++k)
            if (!std::isfinite(s.loglik[k])) return fail(-1, "loglik[%lld, %lld] = %g is not finite", k / s.n_rows, k % s.n_rows, s.loglik[k]);
    return 0;
}
template <class Spec> int pointwise_fit(const ptnn_handle* h, const Spec& s, const RowsByVectors& f) {  // with the handle
    if (int rc = f.fit(h, !s.loglik)) return rc;
    if (!s.loglik && s.x_source == PTNN_PREDICT_X_HOST && h->cfg.task != PTNN_TASK_REG)
        return check_labels(s.x, s.n_rows, h->cfg.n_in, h->cfg.n_out);
    return 0;
}
// The frame's sources on the device: rows with their target, the distinct (w, eta) samples, the forward scratch under `part` of
// $budget_var -- U x (rows x O) floats, + U x rows doubles for loglik_out -- and the sample of every item for loglik_out -> ra
template <class Spec>
int pointwise_stage(ptnn_handle* h, const Spec& s, RowsByVectors& f, const char* budget_var, size_t part, const char* what, ElpdRed* ra) {
    const int I = h->cfg.n_in, O = h->cfg.n_out;
    double* d_llb = nullptr;
    f.eta = true;
    if (int rc = f.stage(h, I + 1, s.n_distinct)) return rc;
    if (int rc = f.forward(h, budget_var, part, (size_t)f.U * (sizeof(float) * O + (s.loglik_out ? sizeof(double) : 0)), s.n_rows, what)) return rc;
    if (s.loglik_out) HIP_TRY(f.mem.alloc(&d_llb, (size_t)f.rows_blk * f.U));
    if (int rc = f.items(h, s.loglik_out != nullptr)) return rc;
    ra->mode = h->cfg.task == PTNN_TASK_REG ? ELPD_REG : ELPD_CLS;
    ra->fx = f.d_fx; ra->eta = f.d.run_eta; ra->y = f.d_x + I; ra->ys = f.xs; ra->cnt = f.d.run_cnt; ra->U = f.U; ra->ll_out = d_llb;
    return 0;
}
// loglik_out of the block of `nr` rows from r0 that `ra` names, in the selection's order
template <class Spec> int pointwise_out(ptnn_handle* h, const Spec& s, const RowsByVectors& f, const ElpdRed& ra, long long r0, int nr) {
    if (int rc = loglik_block(h, ra, nr)) return rc;
    return scatter_samples(h, ra.ll_out, nr, ra.U, f.item_run, f.src.weights(), s.loglik_out, (size_t)s.n_rows, (size_t)r0);
}

// The columns of such a call, `ncols` in all, a block fx [nc][U] at a time: their weighted mean and the order statistics f.rk over the
// samples, and the values of every selected sample in the selection's order.  An output costs device work only when its pointer
// is given.
struct Columns {
    ptnn_handle* h;
    RowsByVectors& f;
    int ncols;
    double* mean;                           // the caller's outputs, each may be null
    float *order_stats, *samples;
    double* d_mean = nullptr;
    int alloc() {
        if (!order_stats) f.rk.n = 0;
        if (mean || order_stats) HIP_TRY(f.mem.alloc(&d_mean, (size_t)ncols));
        return f.rk.to_device(f.mem, (size_t)ncols, h->stream);
    }
    int reduce(const float* fx, long long col0, long long nc) const {
        if (!d_mean) return 0;
        PredictRed ra{fx, f.d.run_cnt, f.U, 1, (int)col0, ncols, f.M, f.rk.n, f.rk.d_ranks, d_mean, f.rk.d_stats, nullptr};
        HIP_TRY(launch(predict_reduce_kernel, dim3((unsigned)nc), dim3(PRED_THREADS), 0, h->stream, ra));
        return 0;
    }
    int scatter(const float* fx, long long col0, long long nc) const {
        return samples ? scatter_samples(h, fx, (int)nc, f.U, f.item_run, f.src.weights(), samples, (size_t)ncols, (size_t)col0) : 0;
    }
    int fetch() const {
        HIP_TRY(::fetch(mean, d_mean, (size_t)ncols, h->stream));
        HIP_TRY(::fetch(order_stats, f.rk.d_stats, (size_t)f.rk.n * ncols, h->stream));
        return 0;
    }
};

// What ptnn_sensitivity and ptnn_coalition_values make of C signed columns per row: per column the mean, order statistics and
// sign counts over the samples; per column of a row (c < C) the weighted mean over the samples of the row means of |.| and (.)^2,
// the exact ranks f.rk2 of the fp32 row mean a_s of |.|, and a_s of every selected sample.
struct SignedColumns {
    ptnn_handle* h;
    RowsByVectors& f;
    int n_rows, C;
    Columns cols;
    int64_t *pos_count, *neg_count;         // the caller's outputs, each may be null
    double *abs_mean, *sq_mean;
    float *abs_order_stats, *sample_abs;
    long long rows_blk = 0;                 // alloc: rows per block, and the block fx [rows_blk * C][U]
    float* fx = nullptr;
    double *d_acc_abs = nullptr, *d_acc_sq = nullptr, *d_abs_mean = nullptr, *d_sq_mean = nullptr, *d_a32_mean = nullptr;
    float* d_a32 = nullptr;
    long long *d_pos = nullptr, *d_neg = nullptr;
    bool signs() const { return pos_count || neg_count; }
    bool sums() const { return abs_mean || sq_mean || abs_order_stats || sample_abs; }
    // fx under the budget $budget_var; ends with the sample of every item queued, where a selection-order output is asked for
    int alloc(const char* budget_var) {
        hipStream_t st = h->stream;
        const int U = f.U;
        if (!abs_order_stats) f.rk2.n = 0;
        HIP_TRY(f.mem.alloc(&d_pos, signs() ? (size_t)cols.ncols : 0));
        HIP_TRY(f.mem.alloc(&d_neg, signs() ? (size_t)cols.ncols : 0));
        if (int rc = cols.alloc()) return rc;
        if (int rc = f.rk2.to_device(f.mem, (size_t)C, st)) return rc;
        if (sums()) {       // per column c and distinct vector: the row sums of |.| and (.)^2, carried across the blocks of rows
            HIP_TRY(f.mem.alloc(&d_acc_abs, (size_t)C * U));
            HIP_TRY(f.mem.alloc(&d_acc_sq, (size_t)C * U));
            HIP_TRY(f.mem.alloc(&d_a32, (size_t)C * U));
            HIP_TRY(f.mem.alloc(&d_abs_mean, (size_t)C));
            HIP_TRY(f.mem.alloc(&d_sq_mean, (size_t)C));
            HIP_TRY(f.mem.alloc(&d_a32_mean, (size_t)C));
            HIP_TRY(hipMemsetAsync(d_acc_abs, 0, (size_t)C * U * sizeof(double), st));
            HIP_TRY(hipMemsetAsync(d_acc_sq, 0, (size_t)C * U * sizeof(double), st));
        }
        rows_blk = row_block(scratch_budget(budget_var), (size_t)U * sizeof(float) * C, n_rows);
        HIP_TRY(f.mem.alloc(&fx, (size_t)rows_blk * C * U));
        return f.items(h, cols.samples || sample_abs);
    }
    // rows [r0, r0 + nr), whose columns the forward pass has left in fx
    int block(long long r0, int nr) const {
        hipStream_t st = h->stream;
        const int U = f.U;
        if (int rc = cols.reduce(fx, r0 * C, (long long)nr * C)) return rc;
        if (signs()) {
            SensSign sa{fx, f.d.run_cnt, U, r0 * C, d_pos, d_neg};
            HIP_TRY(launch(sensitivity_sign_kernel, dim3((unsigned)(nr * C)), dim3(PRED_THREADS), 0, st, sa));
        }
        if (sums()) {
            SensRows rw{fx, U, C, nr, r0 + nr == n_rows ? 1 : 0, (double)n_rows, d_acc_abs, d_acc_sq, d_a32};
            HIP_TRY(launch(sensitivity_rows_kernel, dim3((unsigned)((U + PRED_THREADS - 1) / PRED_THREADS), (unsigned)C), dim3(PRED_THREADS), 0, st, rw));
        }
        return cols.scatter(fx, r0 * C, (long long)nr * C);
    }
    // the weighted means of the row sums (double), the exact ranks of the fp32 a_s, and every output to the caller
    int finish() {
        hipStream_t st = h->stream;
        const int U = f.U;
        if (abs_mean || sq_mean) {
            SensMean ma{d_acc_abs, d_acc_sq, f.d.run_cnt, U, (double)n_rows, f.M, d_abs_mean, d_sq_mean};
            HIP_TRY(launch(sensitivity_mean_kernel, dim3((unsigned)C), dim3(PRED_THREADS), 0, st, ma));
        }
        if (f.rk2.n) {
            PredictRed ra{d_a32, f.d.run_cnt, U, 1, 0, C, f.M, f.rk2.n, f.rk2.d_ranks, d_a32_mean, f.rk2.d_stats, nullptr};
            HIP_TRY(launch(predict_reduce_kernel, dim3((unsigned)C), dim3(PRED_THREADS), 0, st, ra));
        }
        if (sample_abs)
            if (int rc = scatter_samples(h, d_a32, C, U, f.item_run, f.src.weights(), sample_abs, (size_t)C, 0)) return rc;
        if (int rc = cols.fetch()) return rc;
        HIP_TRY(fetch((long long*)pos_count, d_pos, (size_t)cols.ncols, st));
        HIP_TRY(fetch((long long*)neg_count, d_neg, (size_t)cols.ncols, st));
        HIP_TRY(fetch(abs_mean, d_abs_mean, (size_t)C, st));
        HIP_TRY(fetch(sq_mean, d_sq_mean, (size_t)C, st));
        HIP_TRY(fetch(abs_order_stats, f.rk2.d_stats, (size_t)f.rk2.n * C, st));
        return wait_stream(h);
    }
};

// The columns of the predictive mixture (ptnn_dev_calibration.hpp) that ptnn_calibration makes of a regression's data rows and
// ptnn_forecast_score of origins x steps: per column the PIT, mean, sd and quantiles of sum_u c_u N(mu_u, tau_u^2) / S, and its
// CRPS with the all-pairs term.  Spec: the fields the two specs name alike.  With `forecast` the observations are a table of
// their own where NaN marks a column without one: such a column is skipped and keeps the NaN its outputs are filled with first.
template <class Spec> struct MixtureColumns {
    ptnn_handle* h;
    RowsByVectors& f;
    const Spec& s;
    long long ncols;
    bool forecast;
    double *d_tau2 = nullptr, *d_tau = nullptr, *d_itau = nullptr;
    double *d_pit = nullptr, *d_crps = nullptr, *d_mean = nullptr, *d_sd = nullptr, *d_q = nullptr, *d_t1 = nullptr, *d_bound = nullptr;
    unsigned long long* d_limbs = nullptr;
    int n_tiles = 0;
    unsigned n_tri = 0;
    CalibRow ra{};
    CalibPair pa{};
    static int check(const Spec& s) {           // no handle needed
        if (s.n_levels < 0 || s.n_levels > CALIB_MAX_LEVELS) return fail(-1, "n_levels = %d outside [0, %d]", s.n_levels, CALIB_MAX_LEVELS);
        if (s.n_levels > 0 && (!s.levels_p || !s.levels_z || !s.quantiles))
            return fail(-1, "n_levels = %d needs levels_p, levels_z and quantiles", s.n_levels);
        if (s.quantiles && s.n_levels == 0) return fail(-1, "quantiles requested without levels");
        for (int k = 0; k < s.n_levels; ++k)
            if (!(s.levels_p[k] > 0.0 && s.levels_p[k] < 1.0) || !std::isfinite(s.levels_z[k]))
                return fail(-1, "levels_p[%d] = %g (levels_z %g): a quantile level lies in (0, 1)", k, s.levels_p[k], s.levels_z[k]);
        if (s.crps && !s.pair_term) return fail(-1, "crps requested without pair_term");
        return 0;
    }
    hipError_t column(double** p, size_t n) const {                     // a per-column result
        const hipError_t e = f.mem.alloc(p, n);
        return e != hipSuccess || !forecast ? e : hipMemsetAsync(*p, 0xff, n * sizeof(double), h->stream);
    }
    // the results and tau of every distinct sample; mu [nc][U] is the block's image, y the observation of column c at y[c * ys]
    int alloc(const float* mu, const float* y, int ys) {
        hipStream_t st = h->stream;
        const int U = f.U;
        const size_t n = (size_t)ncols;
        HIP_TRY(f.mem.alloc(&d_tau2, (size_t)U));
        HIP_TRY(f.mem.alloc(&d_tau, (size_t)U));
        HIP_TRY(f.mem.alloc(&d_itau, (size_t)U));
        HIP_TRY(column(&d_pit, n));
        HIP_TRY(column(&d_mean, n));
        HIP_TRY(column(&d_sd, n));
        if (s.n_levels) HIP_TRY(column(&d_q, (size_t)s.n_levels * n));
        if (s.pair_term) {
            HIP_TRY(column(&d_crps, n));
            HIP_TRY(column(&d_t1, n));
            HIP_TRY(column(&d_bound, n));
            HIP_TRY(f.mem.alloc(&d_limbs, n * 4));
            HIP_TRY(hipMemsetAsync(d_limbs, 0, n * 4 * sizeof(unsigned long long), st));
        }
        HIP_TRY(launch(calib_tau_kernel, dim3((unsigned)((U + CALIB_THREADS - 1) / CALIB_THREADS)), dim3(CALIB_THREADS), 0, st, U, f.d.run_eta,
                       d_tau2, d_tau, d_itau));
        ra.fx = mu; ra.tau2 = d_tau2; ra.tau = d_tau; ra.itau = d_itau; ra.cnt = f.d.run_cnt; ra.y = y; ra.ys = ys; ra.U = U;
        ra.n_rows = (int)ncols; ra.S = f.M; ra.n_levels = s.n_levels; ra.pair = s.pair_term ? 1 : 0; ra.skip_nan = forecast ? 1 : 0;
        for (int k = 0; k < s.n_levels; ++k) { ra.p[k] = s.levels_p[k]; ra.z[k] = s.levels_z[k]; }
        ra.pit = d_pit; ra.pred_mean = d_mean; ra.pred_sd = d_sd; ra.quantiles = d_q; ra.term1 = d_t1; ra.pair_bound = d_bound;
        n_tiles = (U + CALIB_THREADS - 1) / CALIB_THREADS;
        n_tri = (unsigned)((long long)n_tiles * (n_tiles + 1) / 2);
        pa = CalibPair{mu, d_tau2, f.d.run_cnt, d_bound, U, 0, 0, n_tiles, d_limbs, forecast ? y : nullptr};
        return 0;
    }
    // the columns [col0, col0 + nc), whose image the forward pass has left in mu
    int block(long long col0, int nc) {
        ra.row0 = (int)col0;
        HIP_TRY(launch(calib_row_kernel, dim3((unsigned)nc), dim3(CALIB_THREADS), 0, h->stream, ra));
        // the pair term of this block's columns, at most 65535 (grid.y) per launch
        for (int q0 = 0; s.pair_term && q0 < nc; q0 += 65535) {
            pa.row0 = (int)col0; pa.r0 = q0;
            HIP_TRY(launch(calib_pair_kernel, dim3(n_tri, (unsigned)std::min(65535, nc - q0)), dim3(CALIB_THREADS), 0, h->stream, pa));
        }
        return 0;
    }
    int finish() const {
        if (s.pair_term)
            HIP_TRY(launch(calib_finish_kernel, dim3((unsigned)((ncols + CALIB_THREADS - 1) / CALIB_THREADS)), dim3(CALIB_THREADS), 0, h->stream,
                           (int)ncols, d_limbs, d_t1, d_bound, f.M, d_crps));
        return 0;
    }
    int fetch() const {
        hipStream_t st = h->stream;
        HIP_TRY(::fetch(s.pit, d_pit, (size_t)ncols, st));
        HIP_TRY(::fetch(s.pred_mean, d_mean, (size_t)ncols, st));
        HIP_TRY(::fetch(s.pred_sd, d_sd, (size_t)ncols, st));
        HIP_TRY(::fetch(s.quantiles, d_q, (size_t)s.n_levels * ncols, st));
        HIP_TRY(::fetch(s.crps, d_crps, (size_t)ncols, st));
        return 0;
    }
};

// The votes of the pooled classifier (votes_h on the host): predict_reduce_kernel counts them per column as integers -- exact
// whatever the order -- in `d`; the host divides by the samples.
struct PooledVotes {
    long long* d = nullptr;                 // [ncols], PredictRed's votes; null: a regression
    std::vector<long long> counts;
    hipError_t alloc(DeviceScratch& mem, size_t ncols) { return mem.alloc(&d, ncols); }
    hipError_t fetch(bool wanted, size_t ncols, hipStream_t st) {      // queued: valid after the next wait_stream
        counts.resize(wanted ? ncols : 0);
        return ::fetch(wanted ? counts.data() : nullptr, d, ncols, st);
    }
    double share(size_t c, long long M) const { return (double)counts[c] / (double)M; }
    void shares(double* vote, long long M) const {
        for (size_t c = 0; vote && c < counts.size(); ++c) vote[c] = share(c, M);
    }
};

int modes_cap(long long U) {
    if (U * U > PTNN_MODES_MAX_ELEMENTS)
        return fail(-1, "%lld distinct samples: the %lld x %lld distance matrix exceeds 2^27 elements per call; select fewer samples "
                        "(thin=, chains=)", U, U, U);
    return 0;
}

// What ptnn_modes and ptnn_compress share (include/ptnn.h: ptnn_modes): the three sample sources, the distinct samples' outputs
// F [U][n] and their all-pairs squared distance sq [U][U] (ptnn_dev_modes.hpp), in steps, since the order of the refusals is kept
// and each call has checks and buffers of its own between them.  Spec: the fields the two specs name alike.
template <class Spec> struct SampleDistances {
    const Spec& s;
    const bool mat;                         // source 3
    RowsByVectors f;
    ForwardPlan fwd;
    int U = 0, cpr = 1;                     // cpr: columns per row of x (source 3: per column of values)
    const int* d_cnt = nullptr;             // [U] the counts
    long long rows = 0, n = 0, M = 0, rows_blk = 0;
    bool want_sq = false, want_out = false;
    float *d_fx = nullptr, *d_out = nullptr;
    double* d_sq = nullptr;
    explicit SampleDistances(const Spec& spec) : s(spec), mat(spec.values != nullptr), f(spec, RankOutputs{0, nullptr, nullptr}) {}
    // no handle needed
    int check() {
        if (mat) {
            f.src.host = true;
            if (int rc = check_source(f.src, "samples")) return rc;
            if (s.n_a < 1) return fail(-1, "n_a = %d must be >= 1", s.n_a);
            return modes_cap(s.n_w);                            // every host row is a sample
        }
        return f.check();
    }
    // the samples selected and on the device; `what` names the call
    int stage(ptnn_handle* h, const char* what) {
        if (!mat)
            if (int rc = fit_rows(h, f.rows)) return rc;
        if (int rc = f.select(h, s.n_samples)) return rc;
        if (s.room < f.src.n_items)
            return fail(-1, "room = %lld entries per output but the selection has %lld items", (long long)s.room, f.src.n_items);
        if (mat) {
            int* d_cnt_own = nullptr;
            if (int rc = start_device(h)) return rc;
            f.U = (int)f.src.n_items;
            if (int rc = upload_counts(h, f.mem, s.multiplicity, (size_t)f.U, &d_cnt_own)) return rc;
            if (s.n_distinct) *s.n_distinct = f.U;
            d_cnt = d_cnt_own;
        } else {
            if (int rc = f.stage(h, h->cfg.n_in, s.n_distinct)) return rc;
            if (int rc = modes_cap(f.U)) return rc;
            if (int rc = fwd.init(h, what)) return rc;
            d_cnt = f.d.run_cnt;
        }
        U = f.U; cpr = mat ? 1 : h->cfg.n_out;
        rows = mat ? s.n_a : s.n_rows; n = rows * cpr;
        M = f.M;
        return 0;
    }
    // the column blocks as ptnn_predict cuts them: fx scratch U x (rows x O) floats under the budget; the matrix lies beside it
    int alloc(bool sq) {
        want_sq = sq; want_out = s.outputs && !mat;
        rows_blk = row_block(scratch_budget("PTNN_MODES_SCRATCH_BYTES"), (size_t)U * sizeof(float) * cpr, rows);
        if (want_sq || want_out) HIP_TRY(f.mem.alloc(&d_fx, (size_t)rows_blk * cpr * U));
        if (want_out) HIP_TRY(f.mem.alloc(&d_out, (size_t)U * n));
        if (want_sq) HIP_TRY(f.mem.alloc(&d_sq, (size_t)U * U));
        return 0;
    }
    // `with_items`: the sample of every item is wanted on the host; queues the forward pass and the matrix, block by block
    int form(ptnn_handle* h, bool with_items) {
        hipStream_t st = h->stream;
        if (int rc = f.items(h, with_items && !mat)) return rc;
        // the columns [c0, c0 + nc) of the host matrix [U][n_a] as a block [nc][U] on the device
        std::vector<float> stage;
        auto host_columns = [&](long long c0, int nc) -> int {
            stage.resize((size_t)nc * U);
            for (int c = 0; c < nc; ++c)
                for (int u = 0; u < U; ++u) stage[(size_t)c * U + u] = s.values[(size_t)u * s.n_a + c0 + c];
            HIP_TRY(hipMemcpyAsync(d_fx, stage.data(), stage.size() * sizeof(float), hipMemcpyHostToDevice, st));
            return wait_stream(h);                              // `stage` is written again for the next block
        };
        const int T = (U + MODES_TILE - 1) / MODES_TILE;
        if (!(want_sq || want_out)) return 0;
        return each_block(rows, rows_blk, [&](long long r0, int nr) -> int {
            const int nc = nr * cpr;
            if (mat) {
                if (int rc = host_columns(r0, nc)) return rc;
            } else {
                if (int rc = fwd.run(h, f.d.base, f.d.run_off, f.d_x, f.xs, (int)r0, nr, U, d_fx)) return rc;
            }
            if (want_out) {
                const long long cells = (long long)nc * U;
                HIP_TRY(launch(modes_outputs_kernel, dim3((unsigned)((cells + MODES_THREADS - 1) / MODES_THREADS)), dim3(MODES_THREADS), 0, st,
                               d_fx, n, r0 * cpr, nc, U, d_out));
            }
            if (want_sq) {
                ModesDist da{d_fx, nc, U, T, r0 == 0 ? 1 : 0, d_sq};
                HIP_TRY(launch(modes_dist_kernel, dim3((unsigned)(T * (T + 1) / 2)), dim3(MODES_THREADS), 0, st, da));
            }
            return 0;
        });
    }
    // the sample of item k (after the wait that follows form(with_items))
    int sample_of(long long k) const { return mat ? (int)k : f.item_run[(size_t)k]; }
    // count, sq_dist and outputs queued to the caller
    int fetch_common(hipStream_t st) const {
        HIP_TRY(fetch((int*)s.count, d_cnt, (size_t)U, st));
        HIP_TRY(fetch(s.sq_dist, (const double*)d_sq, (size_t)U * U, st));
        if (want_out) HIP_TRY(fetch(s.outputs, (const float*)d_out, (size_t)U * n, st));
        return 0;
    }
    // behind the last wait: the outputs that are host copies
    void finish() const {
        if (s.outputs && mat) std::copy(s.values, s.values + (size_t)U * n, s.outputs);
        for (long long k = 0; s.item_sample && k < f.src.n_items; ++k) s.item_sample[k] = (int32_t)sample_of(k);
    }
};
}  // namespace

extern "C" {

// ---- posterior predictive (ptnn_dev_predict.hpp) ----
int ptnn_predict(ptnn_handle* h, const ptnn_predict_spec* spec) {
    // argument checks first: none of them needs the handle or a device
    if (int rc = check_spec(spec, "ptnn_predict_spec")) return rc;
    const ptnn_predict_spec& s = *spec;
    RowsByVectors f(s, RankOutputs{s.n_ranks, s.ranks, s.order_stats});
    if (int rc = f.check()) return rc;
    if (int rc = check_handle(h, "ptnn_predict")) return rc;
    const int I = h->cfg.n_in, O = h->cfg.n_out;
    if (s.vote && h->cfg.task != PTNN_TASK_CLS) return fail(-1, "vote: a regression has no classes");
    if (int rc = fit_rows(h, f.rows)) return rc;
    if (int rc = f.select(h, s.n_samples)) return rc;

    if (int rc = f.stage(h, I, s.n_distinct)) return rc;
    hipStream_t st = h->stream;
    DeviceScratch& mem = f.mem;
    const Distinct& d = f.d;
    const RankOutputs& rk = f.rk;
    const long long M = f.M;
    const int U = f.U, ncols = s.n_rows * O;
    // outputs on the device for every column
    double* d_mean = nullptr;
    PooledVotes votes;
    HIP_TRY(mem.alloc(&d_mean, (size_t)ncols));
    if (int rc = f.rk.to_device(mem, (size_t)ncols, st)) return rc;
    if (h->cfg.task == PTNN_TASK_CLS) HIP_TRY(votes.alloc(mem, (size_t)ncols));
    // stage b + c in blocks of rows: fx scratch U x (rows x O) floats under the budget
    if (int rc = f.forward(h, "PTNN_PREDICT_SCRATCH_BYTES", 1, (size_t)U * sizeof(float) * O, s.n_rows, "posterior predictive")) return rc;
    if (int rc = f.items(h, s.samples != nullptr)) return rc;
    if (int rc = f.each_rows(h, s.n_rows, [&](long long r0, int nr) -> int {
        PredictRed ra{f.d_fx, d.run_cnt, U, O, (int)r0 * O, ncols, M, s.n_ranks, rk.d_ranks, d_mean, rk.d_stats, votes.d};
        HIP_TRY(launch(predict_reduce_kernel, dim3((unsigned)(nr * O)), dim3(PRED_THREADS), 0, st, ra));
        return s.samples ? scatter_samples(h, f.d_fx, nr * O, U, f.item_run, f.src.weights(), s.samples, (size_t)s.n_rows * O, (size_t)r0 * O) : 0;
    })) return rc;
    HIP_TRY(fetch(s.mean, d_mean, (size_t)ncols, st));
    HIP_TRY(fetch(s.order_stats, rk.d_stats, (size_t)s.n_ranks * ncols, st));
    HIP_TRY(votes.fetch(s.vote != nullptr, (size_t)ncols, st));
    if (int rc = wait_stream(h)) return rc;
    votes.shares(s.vote, M);
    return 0;
}

// ---- input sensitivity (ptnn_dev_sensitivity.hpp) ----
int ptnn_sensitivity(ptnn_handle* h, const ptnn_sensitivity_spec* spec) {
    // argument checks first: none of them needs the handle or a device
    if (int rc = check_spec(spec, "ptnn_sensitivity_spec")) return rc;
    const ptnn_sensitivity_spec& s = *spec;
    RowsByVectors f(s, RankOutputs{s.n_ranks, s.ranks, s.order_stats}, RankOutputs{s.n_ranks2, s.ranks2, s.abs_order_stats});
    if (int rc = f.check()) return rc;
    if (int rc = check_handle(h, "ptnn_sensitivity")) return rc;
    const int I = h->cfg.n_in, O = h->cfg.n_out, OI = O * I;
    if (int rc = fit_rows(h, f.rows)) return rc;
    const long long ncols_all = (long long)s.n_rows * OI;
    if (ncols_all > 0x7fffffffLL)
        return fail(-1, "%d rows x %d outputs x %d inputs = %lld columns: at most 2^31 - 1 per call", s.n_rows, O, I, ncols_all);
    if (int rc = f.select(h, s.n_samples)) return rc;

    if (int rc = f.stage(h, I, s.n_distinct)) return rc;
    SensPlan fwd;
    if (int rc = fwd.init(h)) return rc;
    // the forward pass, the column reductions and the row sums in blocks of rows: gx scratch U x (rows x O x I) floats under the budget
    SignedColumns g{h, f, s.n_rows, OI, {h, f, (int)ncols_all, s.grad_mean, s.order_stats, s.samples},
                    s.pos_count, s.neg_count, s.abs_mean, s.sq_mean, s.abs_order_stats, s.sample_abs};
    if (int rc = g.alloc("PTNN_SENSITIVITY_SCRATCH_BYTES")) return rc;
    if (int rc = each_block(s.n_rows, g.rows_blk, [&](long long r0, int nr) -> int {
        if (int rc = fwd.run(h, f.d.base, f.d.run_off, f.d_x, f.xs, (int)r0, nr, f.U, g.fx)) return rc;
        return g.block(r0, nr);
    })) return rc;
    return g.finish();
}

// ---- partial dependence and ICE curves (ptnn_dev_pd.hpp) ----
static_assert(PTNN_PD_MAX_GRID == PD_MAX_GRID, "ptnn.h PTNN_PD_MAX_GRID");

static int pd_check_grid(const float* grid, int A, int G) {
    for (int a = 0; a < A; ++a)
        for (int k = 0; k < G; ++k)
            if (!std::isfinite(grid[(size_t)a * G + k]))
                return fail(-1, "grid[%d, %d] = %g (input slot %d, position %d) is not finite", a, k, (double)grid[(size_t)a * G + k], a, k);
    return 0;
}

int ptnn_partial_dependence(ptnn_handle* h, const ptnn_pd_spec* spec) {
    // argument checks first: none of them needs the handle or a device (the grid of inputs == NULL has n_in rows: checked with the handle)
    if (int rc = check_spec(spec, "ptnn_pd_spec")) return rc;
    const ptnn_pd_spec& s = *spec;
    RowsByVectors f(s, RankOutputs{s.n_ranks, s.ranks, s.ice_order_stats},
                    RankOutputs{s.n_ranks2, s.ranks2, s.pd_order_stats ? (const void*)s.pd_order_stats : (const void*)s.range_order_stats});
    if (int rc = f.check()) return rc;
    if (s.n_grid < 1 || s.n_grid > PTNN_PD_MAX_GRID) return fail(-1, "n_grid = %d outside [1, %d]", s.n_grid, PTNN_PD_MAX_GRID);
    if (!s.grid) return fail(-1, "grid is NULL: one row of n_grid values per selected input");
    if (s.inputs && s.n_inputs < 1) return fail(-1, "n_inputs = %d with an input list", s.n_inputs);
    if (s.inputs)
        if (int rc = pd_check_grid(s.grid, s.n_inputs, s.n_grid)) return rc;
    if (int rc = check_handle(h, "ptnn_partial_dependence")) return rc;
    const int I = h->cfg.n_in, O = h->cfg.n_out, G = s.n_grid;
    if (int rc = fit_rows(h, f.rows)) return rc;
    std::vector<int32_t> inputs(s.inputs ? (size_t)s.n_inputs : (size_t)I);
    for (size_t a = 0; a < inputs.size(); ++a) inputs[a] = s.inputs ? s.inputs[a] : (int32_t)a;
    if (!s.inputs)
        if (int rc = pd_check_grid(s.grid, I, G)) return rc;
    std::vector<char> seen((size_t)I, 0);
    for (size_t a = 0; a < inputs.size(); ++a) {
        if (inputs[a] < 0 || inputs[a] >= I) return fail(-1, "inputs[%d] = %d outside [0, %d)", (int)a, inputs[a], I);
        if (seen[(size_t)inputs[a]]) return fail(-1, "inputs[%d] = %d is given twice", (int)a, inputs[a]);
        seen[(size_t)inputs[a]] = 1;
    }
    const int A = (int)inputs.size(), AGO = A * G * O, AO = A * O;
    const long long ncols_all = (long long)s.n_rows * AGO;
    if (ncols_all > 0x7fffffffLL)
        return fail(-1, "%d rows x %d inputs x %d grid values x %d outputs = %lld columns: at most 2^31 - 1 per call", s.n_rows, A, G, O, ncols_all);
    const int ncols = (int)ncols_all;
    if (int rc = f.select(h, s.n_samples)) return rc;

    hipStream_t st = h->stream;
    DeviceScratch& mem = f.mem;
    int* d_inputs = nullptr;
    float* d_grid = nullptr;
    if (int rc = f.stage(h, I, s.n_distinct, [&]() -> int {
        HIP_TRY(mem.upload(&d_inputs, (const int*)inputs.data(), (size_t)A, st));
        HIP_TRY(mem.upload(&d_grid, s.grid, (size_t)A * G, st));
        return 0;
    })) return rc;
    const Distinct& d = f.d;
    const long long M = f.M;
    const int U = f.U;
    // an output costs device work only when its pointer is given
    const bool want_range = s.range_mean || s.range_order_stats || s.sample_range;
    const int nrk_pd = s.pd_order_stats ? s.n_ranks2 : 0, nrk_range = s.range_order_stats ? s.n_ranks2 : 0;
    double *d_acc = nullptr, *d_pd_mean = nullptr, *d_pd32_mean = nullptr, *d_range_mean = nullptr;
    float *d_pd32 = nullptr, *d_range = nullptr, *d_pd_stats = nullptr, *d_range_stats = nullptr;
    long long* d_ranks2 = nullptr;
    Columns ice{h, f, ncols, s.ice_mean, s.ice_order_stats, s.samples};
    if (int rc = ice.alloc()) return rc;
    if (nrk_pd || nrk_range) HIP_TRY(mem.upload(&d_ranks2, (const long long*)s.ranks2, (size_t)s.n_ranks2, st));
    // per (a, k, o) and distinct vector: the row sums of ICE, carried across the blocks of rows
    HIP_TRY(mem.alloc(&d_acc, (size_t)AGO * U));
    HIP_TRY(mem.alloc(&d_pd32, (size_t)AGO * U));
    HIP_TRY(hipMemsetAsync(d_acc, 0, (size_t)AGO * U * sizeof(double), st));
    // the forward pass, the column reductions and the row sums in blocks of rows: fx scratch U x (rows x A x G x O) floats under the budget
    const long long rows_blk = row_block(scratch_budget("PTNN_PD_SCRATCH_BYTES"), (size_t)U * sizeof(float) * AGO, s.n_rows);
    float* d_fx = nullptr;
    HIP_TRY(mem.alloc(&d_fx, (size_t)rows_blk * AGO * U));
    PdPlan fwd;
    if (int rc = fwd.init(h, A, G)) return rc;
    if (int rc = f.items(h, s.samples || s.sample_pd || s.sample_range)) return rc;
    const unsigned ublocks = (unsigned)((U + PRED_THREADS - 1) / PRED_THREADS);
    if (int rc = each_block(s.n_rows, rows_blk, [&](long long r0, int nr) -> int {
        if (int rc = fwd.run(h, d.base, d.run_off, f.d_x, f.xs, (int)r0, nr, U, d_inputs, d_grid, d_fx)) return rc;
        if (int rc = ice.reduce(d_fx, r0 * AGO, (long long)nr * AGO)) return rc;
        PdRows rw{d_fx, U, AGO, nr, r0 + nr == s.n_rows ? 1 : 0, (double)s.n_rows, d_acc, d_pd32};
        HIP_TRY(launch(pd_rows_kernel, dim3(ublocks * (unsigned)AGO), dim3(PRED_THREADS), 0, st, rw));
        return ice.scatter(d_fx, r0 * AGO, (long long)nr * AGO);
    })) return rc;
    // the curve: weighted means of the double row means, exact ranks of PD32; its range per (a, o)
    if (s.pd_mean) {
        HIP_TRY(mem.alloc(&d_pd_mean, (size_t)AGO));
        PdMean ma{d_acc, d.run_cnt, U, (double)s.n_rows, M, d_pd_mean};
        HIP_TRY(launch(pd_mean_kernel, dim3((unsigned)AGO), dim3(PRED_THREADS), 0, st, ma));
    }
    if (nrk_pd) {
        HIP_TRY(mem.alloc(&d_pd32_mean, (size_t)AGO));
        HIP_TRY(mem.alloc(&d_pd_stats, (size_t)nrk_pd * AGO));
        PredictRed ra{d_pd32, d.run_cnt, U, 1, 0, AGO, M, nrk_pd, d_ranks2, d_pd32_mean, d_pd_stats, nullptr};
        HIP_TRY(launch(predict_reduce_kernel, dim3((unsigned)AGO), dim3(PRED_THREADS), 0, st, ra));
    }
    if (want_range) {
        HIP_TRY(mem.alloc(&d_range, (size_t)AO * U));
        PdRange rg{d_pd32, U, A, G, O, d_range};
        HIP_TRY(launch(pd_range_kernel, dim3(ublocks * (unsigned)AO), dim3(PRED_THREADS), 0, st, rg));
        if (s.range_mean || nrk_range) {
            HIP_TRY(mem.alloc(&d_range_mean, (size_t)AO));
            if (nrk_range) HIP_TRY(mem.alloc(&d_range_stats, (size_t)nrk_range * AO));
            PredictRed ra{d_range, d.run_cnt, U, 1, 0, AO, M, nrk_range, d_ranks2, d_range_mean, d_range_stats, nullptr};
            HIP_TRY(launch(predict_reduce_kernel, dim3((unsigned)AO), dim3(PRED_THREADS), 0, st, ra));
        }
    }
    if (s.sample_pd)
        if (int rc = scatter_samples(h, d_pd32, AGO, U, f.item_run, f.src.weights(), s.sample_pd, (size_t)AGO, 0)) return rc;
    if (s.sample_range)
        if (int rc = scatter_samples(h, d_range, AO, U, f.item_run, f.src.weights(), s.sample_range, (size_t)AO, 0)) return rc;
    if (int rc = ice.fetch()) return rc;
    HIP_TRY(fetch(s.pd_mean, d_pd_mean, (size_t)AGO, st));
    HIP_TRY(fetch(s.pd_order_stats, d_pd_stats, (size_t)nrk_pd * AGO, st));
    HIP_TRY(fetch(s.range_mean, d_range_mean, (size_t)AO, st));
    HIP_TRY(fetch(s.range_order_stats, d_range_stats, (size_t)nrk_range * AO, st));
    return wait_stream(h);
}

// ---- accumulated local effects (ptnn_dev_ale.hpp) ----
static_assert(PTNN_ALE_MAX_EDGES == ALE_MAX_EDGES && PTNN_ALE_MAX_EDGES2 == ALE_MAX_EDGES2 && PTNN_ALE_MAX_PAIRS == ALE_MAX_PAIRS,
              "ptnn.h PTNN_ALE limits");

namespace {
// Stage b of the accumulated local effects: the per-shape ale_fwd.  A work-group stages NV distinct vectors in LDS beside their
// finished tiles of one chunk of whole terms: ale_chunk_slots(n_out) slots of two values each, 2 * n_out * 64 floats per slot
// (10 KiB per vector; 18 KiB at n_out = 18, where a pair's two slots are two passes), and once per work-group the chunk's slot
// table (ale_slot_floats); NV = as many vectors as 64 KiB hold (two work-groups share a CU), at most 16.  The largest compiled
// request is 34-512-2: one vector of 18948 floats, a 10-slot chunk and its table, 94 048 B.
struct AlePlan : StagedPlan<AleFwd> {
    int NCH1 = 0, NCH2 = 0;
    int init(const ptnn_handle* h, int A, int Q) {
        const int O = h->cfg.n_out, CS = ale_chunk_slots(O), tile = CS * 2 * O * WAVE;
        vectors(h, ALE_MAX_NV, 64 * 1024 / 4 - ale_slot_floats(O), tile + WAVE);
        NCH1 = (A + CS - 1) / CS;
        NCH2 = (Q + CS / 2 - 1) / (CS / 2);
        return fit(h, "accumulated effects", &AnalysisShape::ale_fwd, tile, (size_t)ale_slot_floats(O));
    }
    // rows [r0, r0 + nr) of x with the terms, edges and outputs `fa` names
    int run(const ptnn_handle* h, AleFwd fa, const float* base, const long long* run_off, const float* x, int xs, int r0, int nr, int U) const {
        fa.c = common(h, base, run_off, x, xs, r0, nr, U);
        fa.VS = VS; fa.NCH1 = NCH1;
        return launch_groups(h, fa, ALE_THREADS, WAVE, NCH1 + NCH2);
    }
};

// `rows` rows of E edges each: finite, z_1 > z_0, strictly increasing and then constant
int ale_check_edges(const char* name, const float* e, int rows, int E) {
    for (int r = 0; r < rows; ++r) {
        const float* z = e + (size_t)r * E;
        for (int k = 0; k < E; ++k)
            if (!std::isfinite(z[k])) return fail(-1, "%s[%d, %d] = %g (row %d, position %d) is not finite", name, r, k, (double)z[k], r, k);
        if (!(z[1] > z[0])) return fail(-1, "%s[%d, 1] = %g <= %s[%d, 0] = %g: the first bin needs a width", name, r, (double)z[1], name, r, (double)z[0]);
        bool flat = false;
        for (int k = 2; k < E; ++k) {
            if (z[k] < z[k - 1]) return fail(-1, "%s[%d, %d] = %g < %s[%d, %d] = %g: edges increase", name, r, k, (double)z[k], name, r, k - 1, (double)z[k - 1]);
            if (z[k] > z[k - 1] && flat)
                return fail(-1, "%s[%d, %d] = %g increases after repeated edges: only the tail may repeat the last edge", name, r, k, (double)z[k]);
            flat = flat || z[k] == z[k - 1];
        }
    }
    return 0;
}

// the columns cols [ncols][U] of the call's second kind: weighted mean, the exact ranks ranks2 and every selected sample's values
int ale_reduce(ptnn_handle* h, RowsByVectors& f, const long long* d_ranks2, int n_ranks2, const float* cols, int ncols, double* mean,
               float* order_stats, float* samples) {
    hipStream_t st = h->stream;
    const int nrk = order_stats ? n_ranks2 : 0;
    if (mean || nrk) {
        double* d_mean = nullptr;
        float* d_stats = nullptr;
        HIP_TRY(f.mem.alloc(&d_mean, (size_t)ncols));
        HIP_TRY(f.mem.alloc(&d_stats, (size_t)nrk * ncols));
        PredictRed ra{cols, f.d.run_cnt, f.U, 1, 0, ncols, f.M, nrk, d_ranks2, d_mean, d_stats, nullptr};
        HIP_TRY(launch(predict_reduce_kernel, dim3((unsigned)ncols), dim3(PRED_THREADS), 0, st, ra));
        HIP_TRY(fetch(mean, d_mean, (size_t)ncols, st));
        HIP_TRY(fetch(order_stats, d_stats, (size_t)nrk * ncols, st));
    }
    return samples ? scatter_samples(h, cols, ncols, f.U, f.item_run, f.src.weights(), samples, (size_t)ncols, 0) : 0;
}
}  // namespace

int ptnn_accumulated_effects(ptnn_handle* h, const ptnn_ale_spec* spec) {
    // argument checks first: none of them needs the handle or a device (the edges of inputs == NULL have n_in rows: checked with the handle)
    if (int rc = check_spec(spec, "ptnn_ale_spec")) return rc;
    const ptnn_ale_spec& s = *spec;
    const void* stats2 = s.ale_order_stats ? (const void*)s.ale_order_stats : s.range_order_stats ? (const void*)s.range_order_stats
                       : s.ale2_order_stats ? (const void*)s.ale2_order_stats : (const void*)s.inter_order_stats;
    RowsByVectors f(s, RankOutputs{s.n_ranks, s.ranks, s.local_order_stats}, RankOutputs{s.n_ranks2, s.ranks2, stats2});
    if (int rc = f.check()) return rc;
    const int Q = s.n_pairs, E = s.n_edges, E2 = s.n_edges2;
    if (Q < 0 || Q > PTNN_ALE_MAX_PAIRS) return fail(-1, "n_pairs = %d outside [0, %d]", Q, PTNN_ALE_MAX_PAIRS);
    if (!s.edges && Q == 0) return fail(-1, "no term: edges is NULL (no first-order input) and n_pairs = 0");
    if (s.edges && (E < 2 || E > PTNN_ALE_MAX_EDGES)) return fail(-1, "n_edges = %d outside [2, %d]", E, PTNN_ALE_MAX_EDGES);
    if (s.edges && s.inputs && s.n_inputs < 1) return fail(-1, "n_inputs = %d with an input list", s.n_inputs);
    if (s.edges && s.inputs)
        if (int rc = ale_check_edges("edges", s.edges, s.n_inputs, E)) return rc;
    if (Q > 0) {
        if (!s.pairs) return fail(-1, "n_pairs = %d but pairs is NULL", Q);
        if (E2 < 2 || E2 > PTNN_ALE_MAX_EDGES2) return fail(-1, "n_edges2 = %d outside [2, %d]", E2, PTNN_ALE_MAX_EDGES2);
        if (!s.edges2) return fail(-1, "edges2 is NULL: two rows of n_edges2 edges per pair");
        if (int rc = ale_check_edges("edges2", s.edges2, 2 * Q, E2)) return rc;
        for (int q = 0; q < Q; ++q) {
            const int j = s.pairs[2 * q], l = s.pairs[2 * q + 1];
            if (j == l) return fail(-1, "pairs[%d] = (%d, %d): a pair needs two different inputs", q, j, l);
            for (int p = 0; p < q; ++p)
                if ((s.pairs[2 * p] == j && s.pairs[2 * p + 1] == l) || (s.pairs[2 * p] == l && s.pairs[2 * p + 1] == j))
                    return fail(-1, "pairs[%d] = (%d, %d) is given twice (pairs[%d])", q, j, l, p);
        }
    }
    if (int rc = check_handle(h, "ptnn_accumulated_effects")) return rc;
    const int I = h->cfg.n_in, O = h->cfg.n_out;
    if (int rc = fit_rows(h, f.rows)) return rc;
    std::vector<int32_t> inputs(!s.edges ? (size_t)0 : s.inputs ? (size_t)s.n_inputs : (size_t)I);
    for (size_t a = 0; a < inputs.size(); ++a) inputs[a] = s.inputs ? s.inputs[a] : (int32_t)a;
    if (s.edges && !s.inputs)
        if (int rc = ale_check_edges("edges", s.edges, I, E)) return rc;
    std::vector<char> seen((size_t)I, 0);
    for (size_t a = 0; a < inputs.size(); ++a) {
        if (inputs[a] < 0 || inputs[a] >= I) return fail(-1, "inputs[%d] = %d outside [0, %d)", (int)a, inputs[a], I);
        if (seen[(size_t)inputs[a]]) return fail(-1, "inputs[%d] = %d is given twice", (int)a, inputs[a]);
        seen[(size_t)inputs[a]] = 1;
    }
    for (int q = 0; q < 2 * Q; ++q)
        if (s.pairs[q] < 0 || s.pairs[q] >= I) return fail(-1, "pairs[%d, %d] = %d outside [0, %d)", q / 2, q % 2, s.pairs[q], I);
    const int A = (int)inputs.size(), T = A + Q, K = A ? E - 1 : 0, K2 = Q ? E2 - 1 : 0, KK = K2 * K2, NB = A * K + Q * KK;
    const int AEO = A * (K + 1) * O, AO = A * O, QEO = Q * (K2 + 1) * (K2 + 1) * O, QO = Q * O;
    const long long ncols_all = (long long)s.n_rows * T * O;
    if (ncols_all > 0x7fffffffLL)
        return fail(-1, "%d rows x %d terms x %d outputs = %lld columns: at most 2^31 - 1 per call", s.n_rows, T, O, ncols_all);
    const int ncols = (int)ncols_all;
    if (int rc = f.select(h, s.n_samples)) return rc;

    hipStream_t st = h->stream;
    DeviceScratch& mem = f.mem;
    int *d_inputs = nullptr, *d_pairs = nullptr;
    float *d_edges = nullptr, *d_edges2 = nullptr;
    if (int rc = f.stage(h, I, s.n_distinct, [&]() -> int {
        if (A) {
            HIP_TRY(mem.upload(&d_inputs, (const int*)inputs.data(), (size_t)A, st));
            HIP_TRY(mem.upload(&d_edges, s.edges, (size_t)A * E, st));
        }
        if (Q) {
            HIP_TRY(mem.upload(&d_pairs, (const int*)s.pairs, (size_t)2 * Q, st));
            HIP_TRY(mem.upload(&d_edges2, s.edges2, (size_t)2 * Q * E2, st));
        }
        return 0;
    })) return rc;
    const Distinct& d = f.d;
    const int U = f.U;
    // an output costs device work only when its pointer is given
    const bool want1 = A && (s.ale_mean || s.ale_order_stats || s.sample_ale || s.range_mean || s.range_order_stats || s.sample_range);
    const bool want2 = Q && (s.ale2_mean || s.ale2_order_stats || s.sample_ale2 || s.inter_mean || s.inter_order_stats || s.sample_inter);
    const bool want_count = s.bin_count || s.cell_count || want1 || want2;
    // what no block size shrinks: the bin accumulators and the surfaces' running sums, per distinct vector
    const size_t budget = scratch_budget("PTNN_ALE_SCRATCH_BYTES");
    const double fixed_bytes = ((want1 || want2 ? (double)NB : 0.0) + (want2 ? (double)QEO / O : 0.0)) * O * U * sizeof(double);
    if (fixed_bytes > (double)std::max(budget, (size_t)1 << 30))
        return fail(-1, "%d bins and cells x %d outputs x %d distinct vectors: the accumulators need %.0f bytes, more than the larger of "
                        "$PTNN_ALE_SCRATCH_BYTES and 1 GiB", NB, O, U, fixed_bytes);
    Columns local{h, f, ncols, s.local_mean, s.local_order_stats, s.samples};
    if (int rc = local.alloc()) return rc;
    long long* d_ranks2 = nullptr;
    if (s.n_ranks2) HIP_TRY(mem.upload(&d_ranks2, (const long long*)s.ranks2, (size_t)s.n_ranks2, st));
    double* d_acc = nullptr;
    int *d_bins = nullptr, *d_count = nullptr;
    HIP_TRY(mem.alloc(&d_bins, (size_t)s.n_rows * T));
    if (want1 || want2) {
        HIP_TRY(mem.alloc(&d_acc, (size_t)NB * O * U));
        HIP_TRY(hipMemsetAsync(d_acc, 0, (size_t)NB * O * U * sizeof(double), st));
    }
    // the forward pass, the column reductions and the bin sums in blocks of rows: fx scratch U x (rows x T x O) floats under the budget
    const long long rows_blk = row_block(budget, (size_t)U * sizeof(float) * T * O, s.n_rows);
    float* d_fx = nullptr;
    HIP_TRY(mem.alloc(&d_fx, (size_t)rows_blk * T * O * U));
    AlePlan fwd;
    if (int rc = fwd.init(h, A, Q)) return rc;
    if (int rc = f.items(h, s.samples || s.sample_ale || s.sample_range || s.sample_ale2 || s.sample_inter)) return rc;
    const unsigned ublocks = (unsigned)((U + PRED_THREADS - 1) / PRED_THREADS);
    AleFwd fa{};
    fa.A = A; fa.Q = Q; fa.E = E; fa.E2 = E2;
    fa.inputs = d_inputs; fa.edges = d_edges; fa.pairs = d_pairs; fa.edges2 = d_edges2; fa.fx = d_fx; fa.bins = d_bins;
    if (int rc = each_block(s.n_rows, rows_blk, [&](long long r0, int nr) -> int {
        if (int rc = fwd.run(h, fa, d.base, d.run_off, f.d_x, f.xs, (int)r0, nr, U)) return rc;
        if (int rc = local.reduce(d_fx, r0 * T * O, (long long)nr * T * O)) return rc;
        if (d_acc) {
            AleBins ba{d_fx, d_bins, U, T, O, A, K, KK, (int)r0, nr, d_acc};
            HIP_TRY(launch(ale_bins_kernel, dim3(ublocks * (unsigned)(T * O)), dim3(PRED_THREADS), 0, st, ba));
        }
        return local.scatter(d_fx, r0 * T * O, (long long)nr * T * O);
    })) return rc;
    std::vector<int32_t> count;
    if (want_count) {       // the rows per bin and cell, once per call
        HIP_TRY(mem.alloc(&d_count, (size_t)NB));
        AleCount ca{d_bins, s.n_rows, T, A, K, KK, NB, d_count};
        HIP_TRY(launch(ale_count_kernel, dim3((unsigned)((NB + PRED_THREADS - 1) / PRED_THREADS)), dim3(PRED_THREADS), 0, st, ca));
        if (s.bin_count || s.cell_count) {
            count.resize((size_t)NB);
            HIP_TRY(fetch(count.data(), (const int32_t*)d_count, (size_t)NB, st));
        }
    }
    if (want1) {            // the curves and their ranges
        float *d_ale32 = nullptr, *d_range = nullptr;
        HIP_TRY(mem.alloc(&d_ale32, (size_t)AEO * U));
        HIP_TRY(mem.alloc(&d_range, (size_t)AO * U));
        AleCurve ca{d_acc, d_count, U, A, K, O, (double)s.n_rows, d_ale32, d_range};
        HIP_TRY(launch(ale_curve_kernel, dim3(ublocks * (unsigned)AO), dim3(PRED_THREADS), 0, st, ca));
        if (int rc = ale_reduce(h, f, d_ranks2, s.n_ranks2, d_ale32, AEO, s.ale_mean, s.ale_order_stats, s.sample_ale)) return rc;
        if (int rc = ale_reduce(h, f, d_ranks2, s.n_ranks2, d_range, AO, s.range_mean, s.range_order_stats, s.sample_range)) return rc;
    }
    if (want2) {            // the surfaces and their interaction strengths
        float *d_ale2 = nullptr, *d_inter = nullptr;
        double* d_work = nullptr;
        HIP_TRY(mem.alloc(&d_ale2, (size_t)QEO * U));
        HIP_TRY(mem.alloc(&d_inter, (size_t)QO * U));
        HIP_TRY(mem.alloc(&d_work, (size_t)QEO * U));
        AleSurface sa{d_acc + (size_t)A * K * O * U, d_count + A * K, U, Q, K2, O, (double)s.n_rows, d_work, d_ale2, d_inter};
        HIP_TRY(launch(ale2_surface_kernel, dim3(ublocks * (unsigned)QO), dim3(PRED_THREADS), 0, st, sa));
        if (int rc = ale_reduce(h, f, d_ranks2, s.n_ranks2, d_ale2, QEO, s.ale2_mean, s.ale2_order_stats, s.sample_ale2)) return rc;
        if (int rc = ale_reduce(h, f, d_ranks2, s.n_ranks2, d_inter, QO, s.inter_mean, s.inter_order_stats, s.sample_inter)) return rc;
    }
    if (int rc = local.fetch()) return rc;
    if (int rc = wait_stream(h)) return rc;
    for (int k = 0; s.bin_count && k < A * K; ++k) s.bin_count[k] = count[(size_t)k];
    for (int k = 0; s.cell_count && k < Q * KK; ++k) s.cell_count[k] = count[(size_t)(A * K + k)];
    return 0;
}

// ---- coalition values: Shapley attributions (ptnn_dev_shapley.hpp) ----
static_assert(PTNN_SHAP_MAX_COALITIONS == SHAP_MAX_COALITIONS && PTNN_SHAP_MAX_BACKGROUND == SHAP_MAX_BACKGROUND &&
              PTNN_SHAP_MAX_TERMS == SHAP_MAX_TERMS && PTNN_SHAP_MAX_ACC == SHAP_MAX_ACC, "ptnn.h PTNN_SHAP limits");
static_assert(SHAP_MAX_ACC % WAVE == 0 && sizeof(unsigned long long) == sizeof(uint64_t), "shapley_forward_kernel: accumulators per lane, masks");

namespace {
// Stage b of the coalition values: the per-shape kernel, NV distinct vectors staged in LDS per work-group -- as many as 64 KiB
// hold, at most SHAP_MAX_NV -- and SHAP_ROWS explained rows; a wave takes (vector, row) pairs
struct ShapPlan : StagedPlan<ShapFwd> {
    int init(const ptnn_handle* h) {
        vectors(h, SHAP_MAX_NV, 64 * 1024 / 4, 0);
        return fit(h, "coalition values", &AnalysisShape::shap_fwd, 0);
    }
    // fx [nr * O * T][U] = the T functionals of vectors base + run_off[u] on rows [r0, r0 + nr) of x
    int run(const ptnn_handle* h, const float* base, const long long* run_off, const float* x, int xs, int r0, int nr, int U,
            const float* bg, int B, int C, int T, const unsigned long long* masks, const double* coef, float* fx) const {
        return launch_groups(h, ShapFwd{common(h, base, run_off, x, xs, r0, nr, U), bg, B, C, T, masks, coef, fx}, SHAP_THREADS, SHAP_ROWS);
    }
};
}  // namespace

int ptnn_coalition_values(ptnn_handle* h, const ptnn_shapley_spec* spec) {
    // argument checks first: none of them needs the handle or a device (a mask's bits are looked at with the handle's n_in)
    if (int rc = check_spec(spec, "ptnn_shapley_spec")) return rc;
    const ptnn_shapley_spec& s = *spec;
    RowsByVectors f(s, RankOutputs{s.n_ranks, s.ranks, s.order_stats}, RankOutputs{s.n_ranks2, s.ranks2, s.abs_order_stats});
    if (int rc = f.check()) return rc;
    if (s.n_background < 1 || s.n_background > PTNN_SHAP_MAX_BACKGROUND)
        return fail(-1, "n_background = %d outside [1, %d]", s.n_background, PTNN_SHAP_MAX_BACKGROUND);
    if (s.n_coalitions < 1 || s.n_coalitions > PTNN_SHAP_MAX_COALITIONS)
        return fail(-1, "n_coalitions = %d outside [1, %d]", s.n_coalitions, PTNN_SHAP_MAX_COALITIONS);
    if (s.n_terms < 1 || s.n_terms > PTNN_SHAP_MAX_TERMS) return fail(-1, "n_terms = %d outside [1, %d]", s.n_terms, PTNN_SHAP_MAX_TERMS);
    if (!s.background) return fail(-1, "background is NULL: n_background rows of n_in values");
    if (!s.masks) return fail(-1, "masks is NULL: one 64-bit mask per coalition");
    if (!s.coef) return fail(-1, "coef is NULL: one row of n_terms coefficients per coalition");
    const int B = s.n_background, C = s.n_coalitions, T = s.n_terms;
    for (int c = 0; c < C; ++c)
        for (int t = 0; t < T; ++t)
            if (!std::isfinite(s.coef[(size_t)c * T + t]))
                return fail(-1, "coef[%d, %d] = %g (coalition %d, term %d) is not finite", c, t, s.coef[(size_t)c * T + t], c, t);
    if (int rc = check_handle(h, "ptnn_coalition_values")) return rc;
    const int I = h->cfg.n_in, O = h->cfg.n_out, OT = O * T;
    if (int rc = fit_rows(h, f.rows)) return rc;
    if (OT > PTNN_SHAP_MAX_ACC) return fail(-1, "n_terms = %d x n_out = %d = %d accumulators: at most %d", T, O, OT, PTNN_SHAP_MAX_ACC);
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < I; ++i)
            if (!std::isfinite(s.background[(size_t)b * I + i]))
                return fail(-1, "background[%d, %d] = %g is not finite", b, i, (double)s.background[(size_t)b * I + i]);
    for (int c = 0; c < C; ++c)
        if (I < 64 && (s.masks[c] >> I) != 0)
            return fail(-1, "masks[%d] = 0x%llx has a bit at or above n_in = %d", c, (unsigned long long)s.masks[c], I);
    const long long ncols_all = (long long)s.n_rows * OT;
    if (ncols_all > 0x7fffffffLL)
        return fail(-1, "%d rows x %d outputs x %d terms = %lld columns: at most 2^31 - 1 per call", s.n_rows, O, T, ncols_all);
    if (int rc = f.select(h, s.n_samples)) return rc;

    float* d_bg = nullptr;
    unsigned long long* d_masks = nullptr;
    double* d_coef = nullptr;
    if (int rc = f.stage(h, I, s.n_distinct, [&]() -> int {
        HIP_TRY(f.mem.upload(&d_bg, s.background, (size_t)B * I, h->stream));
        HIP_TRY(f.mem.upload(&d_masks, (const unsigned long long*)s.masks, (size_t)C, h->stream));
        HIP_TRY(f.mem.upload(&d_coef, s.coef, (size_t)C * T, h->stream));
        return 0;
    })) return rc;
    ShapPlan fwd;
    if (int rc = fwd.init(h)) return rc;
    // the forward pass, the column reductions and the row sums in blocks of rows: fx scratch U x (rows x O x T) floats under the budget
    // (sensitivity_rows_kernel also sums out^2, which is not read: no sq_mean)
    SignedColumns v{h, f, s.n_rows, OT, {h, f, (int)ncols_all, s.mean, s.order_stats, s.samples},
                    s.pos_count, s.neg_count, s.abs_mean, nullptr, s.abs_order_stats, s.sample_abs};
    if (int rc = v.alloc("PTNN_SHAP_SCRATCH_BYTES")) return rc;
    if (int rc = each_block(s.n_rows, v.rows_blk, [&](long long r0, int nr) -> int {
        if (int rc = fwd.run(h, f.d.base, f.d.run_off, f.d_x, f.xs, (int)r0, nr, f.U, d_bg, B, C, T, d_masks, d_coef, v.fx)) return rc;
        return v.block(r0, nr);
    })) return rc;
    return v.finish();
}

// ---- convergence diagnostics (ptnn_dev_convergence.hpp) ----
static_assert(PTNN_TR_LIKEH == TR_LIKEH && PTNN_TR_ACC_TE == TR_ACC_TE && PTNN_TR_ACCEPT == TR_ACCEPT && PTNN_TR_SRC == TR_SRC, "ptnn.h TR order");

// split-R-hat / split-ESS of Q quantities over C chains of n draws, gathered by `ga` (its source fields set: trace rows, or
// draws [C][n][Q] in device memory); outputs are host arrays, any may be null: an output is computed and copied exactly when its
// pointer is given, so ess_chain selects the per-chain ESS and every caller gives rho exactly when n_lags > 0 (ptnn_convergence
// checks it; ptnn_evidence passes neither).  Shared by ptnn_convergence, ptnn_evidence and ptnn_rank_convergence, whose `ga` names a
// double series [C][n][Q] (ga.series) and which gives the scratch `budget` in bytes (0: $PTNN_CONVERGENCE_SCRATCH_BYTES); without ess,
// trunc_lag, ess_chain and rho no lag sum is formed.
static int conv_drive(ptnn_handle* h, DeviceScratch& mem, ConvGather ga, const std::vector<int>& qcol, int C, int n, int n_lags,
                      double* mean, double* var, double* r_hat, double* ess, int32_t* trunc_lag, double* ess_chain, double* rho,
                      size_t budget = 0) {
    const int hl = n / 2, M = 2 * C, Q = (int)qcol.size();
    const bool per_chain = ess_chain != nullptr;
    const bool lags = ess || trunc_lag || ess_chain || n_lags;
    if (!budget) budget = scratch_budget("PTNN_CONVERGENCE_SCRATCH_BYTES");
    const int NS = 1 + (per_chain ? C : 0);
    hipStream_t st = h->stream;
    int *d_qcol = nullptr, *d_error = nullptr;
    HIP_TRY(mem.upload(&d_qcol, qcol.data(), (size_t)Q, st));
    HIP_TRY(mem.alloc(&d_error, 1));
    HIP_TRY(hipMemsetAsync(d_error, 0, sizeof(int), st));
    ga.C = C; ga.n = n; ga.h = hl; ga.error = d_error;
    // outputs of every quantity
    double *d_mean = nullptr, *d_var = nullptr, *d_rhat = nullptr, *d_ess = nullptr, *d_essc = nullptr, *d_rho = nullptr;
    int* d_trunc = nullptr;
    HIP_TRY(mem.alloc(&d_mean, (size_t)Q));
    HIP_TRY(mem.alloc(&d_var, (size_t)Q));
    HIP_TRY(mem.alloc(&d_rhat, (size_t)Q));
    HIP_TRY(mem.alloc(&d_ess, (size_t)Q));
    HIP_TRY(mem.alloc(&d_trunc, (size_t)Q));
    if (per_chain) HIP_TRY(mem.alloc(&d_essc, (size_t)C * Q));
    if (n_lags) HIP_TRY(mem.alloc(&d_rho, (size_t)n_lags * Q));
    // blocks of quantities: the scratch of one quantity, every stage's
    const size_t per_q = sizeof(double) * ((size_t)M * hl + 2 * (size_t)M + 2 * (size_t)C + 2 + (size_t)CONV_MAX_LAGS * C)
                       + sizeof(ConvSeq) * NS + sizeof(int) * (3 + (per_chain ? (size_t)C : 0));
    const int Qb = (int)std::max<size_t>(1, std::min<size_t>(budget / per_q, (size_t)Q));
    double *d_x = nullptr, *d_smean = nullptr, *d_ssq = nullptr, *d_csum = nullptr, *d_cm2 = nullptr, *d_pmean = nullptr, *d_pvar = nullptr;
    double* d_chain = nullptr;
    ConvSeq* d_seq = nullptr;
    int *d_full = nullptr, *d_copen = nullptr, *d_any = nullptr, *d_open = nullptr;
    HIP_TRY(mem.alloc(&d_x, (size_t)Qb * M * hl));
    HIP_TRY(mem.alloc(&d_smean, (size_t)Qb * M));
    HIP_TRY(mem.alloc(&d_ssq, (size_t)Qb * M));
    HIP_TRY(mem.alloc(&d_csum, (size_t)Qb * C));
    HIP_TRY(mem.alloc(&d_cm2, (size_t)Qb * C));
    HIP_TRY(mem.alloc(&d_pmean, (size_t)Qb));
    HIP_TRY(mem.alloc(&d_pvar, (size_t)Qb));
    HIP_TRY(mem.alloc(&d_chain, (size_t)CONV_MAX_LAGS * C * Qb));
    HIP_TRY(mem.alloc(&d_seq, (size_t)Qb * NS));
    HIP_TRY(mem.alloc(&d_full, (size_t)Qb));
    if (per_chain) HIP_TRY(mem.alloc(&d_copen, (size_t)Qb * C));
    HIP_TRY(mem.alloc(&d_any, (size_t)Qb));
    HIP_TRY(mem.alloc(&d_open, (size_t)Qb));
    std::vector<int> any_h((size_t)Qb), open_h((size_t)Qb);
    for (int q0 = 0; q0 < Q; q0 += Qb) {
        const int nq = std::min(Qb, Q - q0);
        // 1. gather and moments
        ga.qcol = d_qcol + q0; ga.nq = nq; ga.x = d_x; ga.smean = d_smean; ga.ssq = d_ssq; ga.csum = d_csum; ga.cm2 = d_cm2;
        HIP_TRY(launch(ga.series ? conv_gather_kernel<true> : conv_gather_kernel<false>, dim3((unsigned)C, (unsigned)((nq + CONV_TILE - 1) / CONV_TILE)),
                       dim3(CONV_THREADS), 0, st, ga));
        // 2. W, var+ and the state of every sequence
        ConvMoments mo{d_smean, d_ssq, d_csum, d_cm2, nq, C, n, hl, NS, d_seq, d_pmean, d_pvar};
        const long long nseq = (long long)nq * NS;
        HIP_TRY(launch(conv_moments_kernel, dim3((unsigned)((nseq + CONV_THREADS - 1) / CONV_THREADS)), dim3(CONV_THREADS), 0, st, mo));
        HIP_TRY(hipMemsetAsync(d_full, 1, (size_t)nq * sizeof(int), st));             // non-zero: every sequence starts open
        if (per_chain) HIP_TRY(hipMemsetAsync(d_copen, 1, (size_t)nq * C * sizeof(int), st));
        int n_open = lags ? nq : 0;
        for (int k = 0; k < nq; ++k) open_h[(size_t)k] = k;
        HIP_TRY(hipMemcpyAsync(d_open, open_h.data(), (size_t)nq * sizeof(int), hipMemcpyHostToDevice, st));
        // 3. blocks of lags, each twice the last, for the quantities with a sequence still open
        for (int t0 = 0, nl = CONV_LAG_TILE; n_open > 0 && t0 < hl; t0 += nl, nl = std::min(2 * nl, CONV_MAX_LAGS)) {
            nl = std::min(nl, (hl - t0 + CONV_LAG_TILE - 1) / CONV_LAG_TILE * CONV_LAG_TILE);
            ConvLags la{d_x, C, hl, d_open, n_open, d_full, d_copen, t0, d_chain};
            HIP_TRY(launch(conv_lags_kernel, dim3((unsigned)((n_open + CONV_TILE - 1) / CONV_TILE), (unsigned)(nl / CONV_LAG_TILE), (unsigned)C),
                           dim3(CONV_THREADS), 0, st, la));
            ConvStep sp{d_chain, d_open, n_open, C, hl, NS, t0, nl, n_lags, Q, q0, d_seq, d_full, d_copen, d_any, d_rho};
            HIP_TRY(launch(conv_step_kernel, dim3((unsigned)n_open), dim3(WAVE), 0, st, sp));
            HIP_TRY(hipMemcpyAsync(any_h.data(), d_any, (size_t)nq * sizeof(int), hipMemcpyDeviceToHost, st));
            if (int rc = wait_stream(h)) return rc;
            const int was_open = n_open;
            n_open = 0;
            for (int k = 0; k < was_open; ++k)
                if (any_h[(size_t)open_h[(size_t)k]]) open_h[(size_t)n_open++] = open_h[(size_t)k];
            if (n_open) HIP_TRY(hipMemcpyAsync(d_open, open_h.data(), (size_t)n_open * sizeof(int), hipMemcpyHostToDevice, st));
        }
        if (n_open) return fail(-2, "%d quantities still open after every lag (internal error)", n_open);
        // 4. tau, ess, r_hat
        ConvFinish fi{d_seq, d_pmean, d_pvar, nq, NS, C, hl, Q, q0, d_mean, d_var, d_rhat, d_ess, d_essc, d_trunc};
        HIP_TRY(launch(conv_finish_kernel, dim3((unsigned)((nseq + CONV_THREADS - 1) / CONV_THREADS)), dim3(CONV_THREADS), 0, st, fi));
    }
    int err = 0;
    HIP_TRY(hipMemcpyAsync(&err, d_error, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(fetch(mean, d_mean, (size_t)Q, st));
    HIP_TRY(fetch(var, d_var, (size_t)Q, st));
    HIP_TRY(fetch(r_hat, d_rhat, (size_t)Q, st));
    HIP_TRY(fetch(ess, d_ess, (size_t)Q, st));
    HIP_TRY(fetch(trunc_lag, d_trunc, (size_t)Q, st));
    HIP_TRY(fetch(ess_chain, d_essc, (size_t)C * Q, st));
    HIP_TRY(fetch(rho, d_rho, (size_t)n_lags * Q, st));
    if (int rc = wait_stream(h)) return rc;
    if (err) return fail(-2, "%d selected compact trace rows refer to rows that are not resident (internal error)", err);
    return 0;
}

// The quantities of ptnn_convergence and ptnn_rank_convergence (one Spec's source fields are the other's), in three parts, since
// each call has checks of its own between them.  conv_check_source: the checks that need no handle.
extern "C++" {
template <class Spec> int conv_check_source(const Spec& s) {
    constexpr int scalar_cols = (1 << TR_LIKEH) | (1 << TR_RMSE_TR) | (1 << TR_RMSE_TE) | (1 << TR_ACC_TR) | (1 << TR_ACC_TE);
    if (s.draws) {
        if (s.n_chains < 1) return fail(-1, "n_chains = %d must be >= 1", s.n_chains);
        if (s.n_draws < 4) return fail(-1, "n_draws = %d: the split chains need at least 4 draws per chain", s.n_draws);
        if (s.n_quantities < 1) return fail(-1, "n_quantities = %d must be >= 1", s.n_quantities);
    } else {
        if (s.thin < 1) return fail(-1, "thin = %d must be >= 1", s.thin);
        if (s.replicas && s.n_replicas < 1) return fail(-1, "n_replicas = %d with a replica list", s.n_replicas);
        if (s.params && s.n_params < 0) return fail(-1, "n_params = %d with a parameter list", s.n_params);
        if (s.scalars & ~scalar_cols)
            return fail(-1, "scalars = 0x%x: only TR_LIKEH, TR_RMSE_TR, TR_RMSE_TE, TR_ACC_TR and TR_ACC_TE are quantities "
                            "(not TR_ACCEPT, TR_LOGALPHA or TR_SRC)", (unsigned)s.scalars);
    }
    return 0;
}
// the selection: chains, draws per chain, the column of every quantity
struct ConvSelection {
    std::vector<int32_t> reps;
    std::vector<int> qcol;
    int C = 0, n = 0;
};
template <class Spec> int conv_select(const ptnn_handle* h, const Spec& s, ConvSelection* sel) {
    const int P = h->P;
    if (s.draws) {
        sel->C = s.n_chains; sel->n = s.n_draws;
        for (int q = 0; q < s.n_quantities; ++q) sel->qcol.push_back(q);
        return 0;
    }
    if (int rc = select_trace_rows(h, s.replicas, s.n_replicas, s.step0, s.nsteps, s.thin, &sel->reps, &sel->n)) return rc;
    sel->C = (int)sel->reps.size();
    if (sel->n < 4) return fail(-1, "%d draws per chain selected: the split chains need at least 4", sel->n);
    if (s.params) {
        for (int k = 0; k < s.n_params; ++k) {
            if (s.params[k] < 0 || s.params[k] >= P) return fail(-1, "parameter %d out of range [0, %d)", s.params[k], P);
            sel->qcol.push_back(s.params[k]);
        }
    } else {
        for (int p = 0; p < P; ++p) sel->qcol.push_back(p);
    }
    for (int c = 0; c < TR_COUNT; ++c)
        if (s.scalars & (1 << c)) sel->qcol.push_back(-1 - c);
    if (sel->qcol.empty()) return fail(-1, "no quantity selected");
    return 0;
}
// the source fields of the gather: the host draws uploaded, or the trace
template <class Spec> int conv_source(ptnn_handle* h, DeviceScratch& mem, const Spec& s, const ConvSelection& sel, ConvGather* ga) {
    hipStream_t st = h->stream;
    if (s.draws) {
        float* d_draws = nullptr;
        const int Q = (int)sel.qcol.size();
        HIP_TRY(mem.upload(&d_draws, s.draws, (size_t)sel.C * sel.n * Q, st));
        ga->host = 1; ga->draws = d_draws; ga->Qh = Q;
    } else {
        int* d_reps = nullptr;
        HIP_TRY(mem.upload(&d_reps, sel.reps.data(), sel.reps.size(), st));
        ga->host = 0; ga->pos_w = h->d_pos_w; ga->scal = h->d_scal; ga->replicas = d_reps; ga->cap = h->cap; ga->PW = h->PW;
        ga->step0 = s.step0; ga->thin = s.thin; ga->compact = h->plan.compact ? 1 : 0;
    }
    return 0;
}
}  // extern "C++"

int ptnn_convergence(ptnn_handle* h, const ptnn_convergence_spec* spec) {
    // argument checks first: none of them needs the handle or a device
    if (int rc = check_spec(spec, "ptnn_convergence_spec")) return rc;
    const ptnn_convergence_spec& s = *spec;
    if (int rc = conv_check_source(s)) return rc;
    if (s.n_lags < 0) return fail(-1, "n_lags = %d must be >= 0", s.n_lags);
    if (s.n_lags > 0 && !s.rho) return fail(-1, "n_lags = %d but rho is NULL", s.n_lags);
    if (s.rho && s.n_lags == 0) return fail(-1, "rho requested with n_lags = 0");
    if (int rc = check_handle(h, "ptnn_convergence")) return rc;
    ConvSelection sel;
    if (int rc = conv_select(h, s, &sel)) return rc;
    if (s.n_lags > sel.n / 2) return fail(-1, "n_lags = %d exceeds the split-chain length %d", s.n_lags, sel.n / 2);

    if (int rc = start_device(h)) return rc;
    DeviceScratch mem;
    ConvGather ga{};
    if (int rc = conv_source(h, mem, s, sel, &ga)) return rc;
    return conv_drive(h, mem, ga, sel.qcol, sel.C, sel.n, s.n_lags, s.mean, s.var, s.r_hat, s.ess, s.trunc_lag, s.ess_chain, s.rho);
}

// ---- rank-normalised convergence diagnostics (ptnn_dev_rank.hpp) ----
static_assert(PTNN_RANK_MAX_BINS * 128 == RANK_HIST_LDS, "the LDS histogram holds 128 chains at the largest bin count");

// the segmented bitonic sort of ptnn_dev_powerscale.hpp: every one of the `nseg` segments of npow words ascending
static int sort_segments(ptnn_handle* h, unsigned long long* keys, int nseg, int npow) {
    hipStream_t st = h->stream;
    const int tile = std::min(npow, PS_SORT_TILE);
    const dim3 tiles((unsigned)(npow / tile), (unsigned)nseg);
    HIP_TRY(launch(powerscale_sort_lds_kernel, tiles, dim3(PS_THREADS), 0, st, keys, npow, tile, 2, tile));
    for (int size = 2 * tile; size <= npow; size <<= 1) {
        for (int stride = size / 2; stride >= tile; stride >>= 1)
            HIP_TRY(launch(powerscale_sort_step_kernel, dim3((unsigned)((npow / 2 + PS_THREADS - 1) / PS_THREADS), (unsigned)nseg), dim3(PS_THREADS),
                           0, st, keys, npow, size, stride));
        HIP_TRY(launch(powerscale_sort_lds_kernel, tiles, dim3(PS_THREADS), 0, st, keys, npow, tile, size, size));
    }
    return 0;
}

int ptnn_rank_convergence(ptnn_handle* h, const ptnn_rank_convergence_spec* spec) {
    // argument checks first: none of them needs the handle or a device
    if (int rc = check_spec(spec, "ptnn_rank_convergence_spec")) return rc;
    const ptnn_rank_convergence_spec& s = *spec;
    if (int rc = conv_check_source(s)) return rc;
    if (s.n_probs < 0 || s.n_probs > PTNN_RANK_MAX_PROBS) return fail(-1, "n_probs = %d outside [0, %d]", s.n_probs, PTNN_RANK_MAX_PROBS);
    if (s.n_probs > 0 && !s.probs) return fail(-1, "n_probs = %d but probs is NULL", s.n_probs);
    for (int k = 0; k < s.n_probs; ++k)
        if (!(s.probs[k] > 0.0 && s.probs[k] < 1.0)) return fail(-1, "probs[%d] = %g must lie in (0, 1)", k, s.probs[k]);
    if (s.ess_quantile && s.n_probs == 0) return fail(-1, "ess_quantile requested with n_probs = 0");
    if (s.n_bins < 2 || s.n_bins > PTNN_RANK_MAX_BINS) return fail(-1, "n_bins = %d outside [2, %d]", s.n_bins, PTNN_RANK_MAX_BINS);
    if (int rc = check_handle(h, "ptnn_rank_convergence")) return rc;
    ConvSelection sel;
    if (int rc = conv_select(h, s, &sel)) return rc;
    const int C = sel.C, n = sel.n, hl = n / 2, Q = (int)sel.qcol.size(), B = s.n_bins;
    if (C > RANK_MAX_GRID_Y || 2LL * C * hl > RANK_MAX_POOLED)
        return fail(-1, "%d chains of %d kept draws: at most 65535 chains and 2^29 pooled draws per quantity", C, 2 * hl);
    const bool chain_out = s.ess_bulk_chain || s.ess_tail_chain;
    const RankPlan plan = rank_plan(C, hl, Q, chain_out, scratch_budget("PTNN_CONVERGENCE_SCRATCH_BYTES"));
    const int L = (int)plan.L, Qb = plan.Qb;

    if (int rc = start_device(h)) return rc;
    hipStream_t st = h->stream;
    DeviceScratch mem;
    RankGather ga{};
    if (int rc = conv_source(h, mem, s, sel, &ga.src)) return rc;
    int *d_qcol = nullptr, *d_error = nullptr, *d_bad = nullptr;
    unsigned long long *d_keys = nullptr, *d_hist = nullptr;
    double* d_ser = nullptr;
    HIP_TRY(mem.upload(&d_qcol, sel.qcol.data(), (size_t)Q, st));
    HIP_TRY(mem.alloc(&d_error, 1));
    HIP_TRY(mem.alloc(&d_bad, (size_t)Q));
    HIP_TRY(hipMemsetAsync(d_error, 0, sizeof(int), st));
    HIP_TRY(hipMemsetAsync(d_bad, 0, (size_t)Q * sizeof(int), st));
    if (s.rank_hist) {
        HIP_TRY(mem.alloc(&d_hist, (size_t)C * B * Q));
        HIP_TRY(hipMemsetAsync(d_hist, 0, (size_t)C * B * Q * sizeof(unsigned long long), st));
    }
    HIP_TRY(mem.alloc(&d_keys, plan.key_words * Qb));
    HIP_TRY(mem.alloc(&d_ser, (size_t)L * Qb));
    ga.src.C = C; ga.src.n = n; ga.src.h = hl; ga.src.error = d_error;

    // the probabilities of the indicator series: 0.05, 0.95 (ess_tail), 0.5 (ess_median), then the caller's
    std::vector<double> probs{0.05, 0.95, 0.5};
    probs.insert(probs.end(), s.probs, s.probs + s.n_probs);
    const double nan = std::nan("");
    std::vector<double> ess_q(probs.size() * (size_t)Q, nan), tmp;
    std::vector<int> cols;
    // one series of every segment of the block [q0, q0 + nq) -> its split-R-hat and split-ESS, to r_hat / ess [width] at q0 (the
    // per-chain segments: chain-major, to [C][width])
    auto series = [&](int q0, int nq, bool per_chain, int mode, int lo, double* r_hat, double* ess, size_t width) -> int {
        const int nseg = per_chain ? nq * C : nq, Ls = per_chain ? 2 * hl : L;
        RankSeries ra{d_keys, d_bad + q0, mode, lo, Ls, (int)(per_chain ? plan.npow_chain : plan.npow), nq, C, per_chain ? 1 : 0, d_ser,
                      per_chain ? nullptr : d_hist, B, Q, q0};
        // LDS for the histogram counters only where this launch counts and they fit (rank_series_kernel's `count && in_lds`)
        const size_t lds = mode == RANK_BULK && ra.hist && C * B <= RANK_HIST_LDS ? (size_t)C * B * sizeof(int) : 0;
        HIP_TRY(launch(rank_series_kernel, dim3((unsigned)((Ls + RANK_THREADS - 1) / RANK_THREADS), (unsigned)nseg), dim3(RANK_THREADS), lds, st, ra));
        if (!r_hat && !ess) return 0;
        ConvGather cg{};
        cg.host = 1; cg.series = d_ser; cg.Qh = nseg;
        cols.resize((size_t)nseg);
        for (int k = 0; k < nseg; ++k) cols[(size_t)k] = k;
        tmp.assign(2 * (size_t)nseg, nan);
        DeviceScratch cm;                                   // conv_drive's buffers: released before the next series
        if (int rc = conv_drive(h, cm, cg, cols, per_chain ? 1 : C, 2 * hl, 0, nullptr, nullptr, r_hat ? tmp.data() : nullptr,
                                ess ? tmp.data() + nseg : nullptr, nullptr, nullptr, nullptr, plan.conv_budget)) return rc;
        for (int c = 0; c < (per_chain ? C : 1); ++c)
            for (int k = 0; k < nq; ++k) {
                if (r_hat) r_hat[(size_t)c * width + q0 + k] = tmp[(size_t)c * nq + k];
                if (ess) ess[(size_t)c * width + q0 + k] = tmp[(size_t)nseg + (size_t)c * nq + k];
            }
        return 0;
    };
    // a sort of the block's segments: the padding filled, the words gathered, every segment ordered
    auto sorted = [&](int q0, int nq, bool per_chain) -> int {
        const int nseg = per_chain ? nq * C : nq, npow = (int)(per_chain ? plan.npow_chain : plan.npow);
        HIP_TRY(hipMemsetAsync(d_keys, 0xff, (size_t)nseg * npow * sizeof(unsigned long long), st));
        ga.src.qcol = d_qcol + q0; ga.src.nq = nq; ga.per_chain = per_chain ? 1 : 0; ga.npow = npow; ga.keys = d_keys; ga.bad = d_bad + q0;
        HIP_TRY(launch(rank_gather_kernel, dim3((unsigned)C, (unsigned)((nq + RANK_TILE - 1) / RANK_TILE)), dim3(RANK_THREADS), 0, st, ga));
        return sort_segments(h, d_keys, nseg, npow);
    };
    std::vector<double> essc_q(chain_out && s.ess_tail_chain ? 2 * (size_t)C * Q : 0, nan);
    const bool any_q = s.ess_tail || s.ess_median || s.ess_quantile;
    if (s.r_hat_bulk || s.ess_bulk || s.r_hat_tail || s.z || s.rank_hist || any_q)
        if (int rc = each_block(Q, Qb, [&](long long q0l, int nq) -> int {
            const int q0 = (int)q0l;
            if (int rc = sorted(q0, nq, false)) return rc;
            if (s.r_hat_bulk || s.ess_bulk || s.z || s.rank_hist) {
                if (int rc = series(q0, nq, false, RANK_BULK, 0, s.r_hat_bulk, s.ess_bulk, (size_t)Q)) return rc;
                if (s.z) {
                    HIP_TRY(hipMemcpy2DAsync(s.z + q0, (size_t)Q * sizeof(double), d_ser, (size_t)nq * sizeof(double), (size_t)nq * sizeof(double),
                                             (size_t)L, hipMemcpyDeviceToHost, st));
                    if (int rc = wait_stream(h)) return rc;
                }
            }
            if (s.r_hat_tail)
                if (int rc = series(q0, nq, false, RANK_FOLD, 0, s.r_hat_tail, nullptr, (size_t)Q)) return rc;
            for (size_t k = 0; k < probs.size(); ++k) {
                if (!(k < 2 ? s.ess_tail != nullptr : k == 2 ? s.ess_median != nullptr : s.ess_quantile != nullptr)) continue;
                const int lo = (int)std::floor((double)(L - 1) * probs[k]);
                if (int rc = series(q0, nq, false, RANK_INDICATOR, lo, nullptr, ess_q.data() + k * (size_t)Q, (size_t)Q)) return rc;
            }
            return 0;
        })) return rc;
    if (chain_out)
        if (int rc = each_block(Q, plan.Qb_chain, [&](long long q0l, int nq) -> int {
            const int q0 = (int)q0l, Lc = 2 * hl;
            if (int rc = sorted(q0, nq, true)) return rc;
            if (s.ess_bulk_chain)
                if (int rc = series(q0, nq, true, RANK_BULK, 0, nullptr, s.ess_bulk_chain, (size_t)Q)) return rc;
            for (size_t k = 0; k < 2 && s.ess_tail_chain; ++k) {
                const int lo = (int)std::floor((double)(Lc - 1) * probs[k]);
                if (int rc = series(q0, nq, true, RANK_INDICATOR, lo, nullptr, essc_q.data() + k * (size_t)C * Q, (size_t)Q)) return rc;
            }
            return 0;
        })) return rc;
    int err = 0;
    std::vector<int> bad((size_t)Q);
    HIP_TRY(hipMemcpyAsync(&err, d_error, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(bad.data(), d_bad, (size_t)Q * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(fetch((unsigned long long*)s.rank_hist, d_hist, (size_t)C * B * Q, st));
    if (int rc = wait_stream(h)) return rc;
    if (err) return fail(-2, "%d selected compact trace rows refer to rows that are not resident (internal error)", err);
    // the smaller of two ESS, NaN if either is; a quantity with a draw that is not finite has NaN everywhere
    auto lesser = [](double a, double b) { return std::isnan(a) || std::isnan(b) ? std::nan("") : std::min(a, b); };
    for (int q = 0; q < Q; ++q) {
        const bool ok = !bad[(size_t)q];
        if (s.ess_tail) s.ess_tail[q] = ok ? lesser(ess_q[(size_t)q], ess_q[(size_t)Q + q]) : nan;
        if (s.ess_median) s.ess_median[q] = ok ? ess_q[2 * (size_t)Q + q] : nan;
        for (int k = 0; s.ess_quantile && k < s.n_probs; ++k) s.ess_quantile[(size_t)k * Q + q] = ok ? ess_q[(size_t)(3 + k) * Q + q] : nan;
        for (int c = 0; c < C; ++c) {
            const size_t o = (size_t)c * Q + q;
            if (s.ess_tail_chain) s.ess_tail_chain[o] = ok ? lesser(essc_q[o], essc_q[(size_t)C * Q + o]) : nan;
            if (s.ess_bulk_chain && !ok) s.ess_bulk_chain[o] = nan;
        }
        if (ok) continue;
        if (s.r_hat_bulk) s.r_hat_bulk[q] = nan;
        if (s.r_hat_tail) s.r_hat_tail[q] = nan;
        if (s.ess_bulk) s.ess_bulk[q] = nan;
    }
    return 0;
}

// ---- predictive accuracy (ptnn_dev_elpd.hpp) ----
static_assert(PTNN_ELPD_TAIL_CAP == ELPD_TAIL_CAP, "ptnn.h tail capacity");

int ptnn_elpd(ptnn_handle* h, const ptnn_elpd_spec* spec) {
    // argument checks first: none of them needs the handle or a device
    if (int rc = check_spec(spec, "ptnn_elpd_spec")) return rc;
    const ptnn_elpd_spec& s = *spec;
    const bool ll_src = s.loglik != nullptr;
    RowsByVectors f(s, x_rows(s), ll_src || s.w != nullptr);
    if (int rc = pointwise_source(s, f)) return rc;
    if (int rc = pointwise_rows(s, f)) return rc;
    if (int rc = check_handle(h, "ptnn_elpd")) return rc;
    if (int rc = pointwise_fit(h, s, f)) return rc;
    if (int rc = f.select(h, nullptr, "p_waic (a variance, ddof 1) needs at least 2")) return rc;
    const long long n_items = f.src.n_items, S = f.M;
    long long M = 0;
    if (int rc = psis_tail(S, s.r_eff, &M)) return rc;
    if (s.n_samples) *s.n_samples = S;

    if (int rc = f.start(h)) return rc;
    hipStream_t st = h->stream;
    DeviceScratch& mem = f.mem;
    const int n_rows = s.n_rows;
    double *d_lppd = nullptr, *d_pwaic = nullptr, *d_loo = nullptr, *d_khat = nullptr;
    long long* d_tail = nullptr;
    HIP_TRY(mem.alloc(&d_lppd, (size_t)n_rows));
    HIP_TRY(mem.alloc(&d_pwaic, (size_t)n_rows));
    HIP_TRY(mem.alloc(&d_loo, (size_t)n_rows));
    HIP_TRY(mem.alloc(&d_khat, (size_t)n_rows));
    HIP_TRY(mem.alloc(&d_tail, (size_t)n_rows));
    ElpdRed ra{};
    ra.O = h->cfg.n_out; ra.S = S; ra.M = (int)M;
    ra.lppd = d_lppd; ra.p_waic = d_pwaic; ra.elpd_loo = d_loo; ra.khat = d_khat; ra.tail_len = d_tail;
    auto copy_out = [&]() -> int {
        HIP_TRY(fetch(s.lppd, d_lppd, (size_t)n_rows, st));
        HIP_TRY(fetch(s.p_waic, d_pwaic, (size_t)n_rows, st));
        HIP_TRY(fetch(s.elpd_loo, d_loo, (size_t)n_rows, st));
        HIP_TRY(fetch(s.khat, d_khat, (size_t)n_rows, st));
        HIP_TRY(fetch((long long*)s.tail_len, d_tail, (size_t)n_rows, st));
        return wait_stream(h);
    };

    if (ll_src) {
        if (int rc = upload_loglik(h, mem, s, n_items, &ra)) return rc;
        HIP_TRY(launch(elpd_reduce_kernel, dim3((unsigned)n_rows), dim3(ELPD_THREADS), 0, st, ra));
        if (s.n_distinct) *s.n_distinct = n_items;
        return copy_out();
    }

    // stage a: the rows with their targets, items -> distinct (w, eta) samples; stages b + c in blocks of rows
    if (int rc = pointwise_stage(h, s, f, "PTNN_ELPD_SCRATCH_BYTES", 1, "predictive accuracy", &ra)) return rc;
    if (int rc = f.each_rows(h, n_rows, [&](long long r0, int nr) -> int {
        ra.row0 = (int)r0;
        HIP_TRY(launch(elpd_reduce_kernel, dim3((unsigned)nr), dim3(ELPD_THREADS), 0, st, ra));
        return s.loglik_out ? pointwise_out(h, s, f, ra, r0, nr) : 0;
    })) return rc;
    return copy_out();
}

// ---- leave-future-out cross-validation (ptnn_dev_lfo.hpp) ----
int ptnn_lfo(ptnn_handle* h, const ptnn_lfo_spec* spec) {
    // argument checks first: none of them needs the handle or a device
    if (int rc = check_spec(spec, "ptnn_lfo_spec")) return rc;
    const ptnn_lfo_spec& s = *spec;
    const bool ll_src = s.loglik != nullptr;
    RowsByVectors f(s, x_rows(s), ll_src || s.w != nullptr);
    if (int rc = pointwise_source(s, f)) return rc;
    if (s.block < 1) return fail(-1, "block = %d must be >= 1", s.block);
    if (s.n_fit < 1 || s.n_fit > s.n_rows)
        return fail(-1, "n_fit = %d outside [1, %d]: the samples are conditioned on rows [0, n_fit) of the %d rows", s.n_fit, s.n_rows, s.n_rows);
    if (s.n_origins < 1 || !s.origins) return fail(-1, "n_origins = %d origins%s: need at least one", s.n_origins, s.origins ? "" : " (origins is NULL)");
    for (int k = 0; k < s.n_origins; ++k) {
        const long long i = s.origins[k];
        if (i < 1 || i >= s.n_rows) return fail(-1, "origin %lld (origins[%d]) outside [1, %d): an origin predicts from the rows before it", i, k, s.n_rows);
        if (i + s.block > s.n_rows)
            return fail(-1, "origin %lld (origins[%d]) with block = %d: i + block > n_rows = %d", i, k, s.block, s.n_rows);
    }
    if (int rc = pointwise_rows(s, f)) return rc;
    if (int rc = check_handle(h, "ptnn_lfo")) return rc;
    if (int rc = pointwise_fit(h, s, f)) return rc;
    if (int rc = f.select(h, nullptr, "importance weights need at least 2")) return rc;
    const long long n_items = f.src.n_items, S = f.M;
    long long M = 0;
    if (int rc = psis_tail(S, s.r_eff, &M)) return rc;
    if (s.n_samples) *s.n_samples = S;

    if (int rc = f.start(h)) return rc;
    hipStream_t st = h->stream;
    DeviceScratch& mem = f.mem;
    const int n_rows = s.n_rows, n_org = s.n_origins;
    double *d_lfo = nullptr, *d_khat = nullptr;
    long long* d_tail = nullptr;
    HIP_TRY(mem.alloc(&d_lfo, (size_t)n_org));
    HIP_TRY(mem.alloc(&d_khat, (size_t)n_org));
    HIP_TRY(mem.alloc(&d_tail, (size_t)n_org));
    if (int rc = raise_lds_limit(reinterpret_cast<const void*>(lfo_reduce_kernel), LFO_LDS_BYTES)) return rc;

    // The samples: source 3 as it is (every host sample its own entry), else stage a.  The budget: half for the sums C (the columns
    // n_fit, i and i + block of a pass of origins), half for a block of rows
    LfoAcc acc{};
    ElpdRed& ra = acc.a;
    ra.O = h->cfg.n_out; ra.S = S; ra.M = (int)M;
    if (ll_src) {
        if (int rc = upload_loglik(h, mem, s, n_items, &ra)) return rc;
        if (s.n_distinct) *s.n_distinct = ra.U;
    } else {
        if (int rc = pointwise_stage(h, s, f, "PTNN_LFO_SCRATCH_BYTES", 2, "leave-future-out", &ra)) return rc;
    }
    const int U = ra.U;
    const long long cols_fit = (long long)((scratch_budget("PTNN_LFO_SCRATCH_BYTES") / 2) / ((size_t)U * sizeof(double)));
    const int org_pass = (int)std::max(1LL, std::min<long long>((cols_fit - 1) / 2, n_org));
    const int max_slots = 2 * org_pass + 1;
    double *d_C = nullptr, *d_carry = nullptr;
    int *d_slot_of = nullptr, *d_org_slot = nullptr;
    HIP_TRY(mem.alloc(&d_C, (size_t)max_slots * U));
    HIP_TRY(mem.alloc(&d_carry, (size_t)U));
    HIP_TRY(mem.alloc(&d_slot_of, (size_t)n_rows + 1));
    HIP_TRY(mem.alloc(&d_org_slot, (size_t)2 * org_pass));
    acc.slot_of = d_slot_of; acc.carry = d_carry; acc.C = d_C;
    std::vector<int> slot_of((size_t)n_rows + 1), org_slot((size_t)2 * org_pass);
    const unsigned acc_blocks = (unsigned)((U + ELPD_THREADS - 1) / ELPD_THREADS);

    for (int o0 = 0; o0 < n_org; o0 += org_pass) {
        const int no = std::min(org_pass, n_org - o0);
        // the columns of this pass, and the last row any of them sums
        std::fill(slot_of.begin(), slot_of.end(), -1);
        int n_slots = 0, n_end = s.n_fit;
        auto slot = [&](int j) { if (slot_of[(size_t)j] < 0) slot_of[(size_t)j] = n_slots++; return slot_of[(size_t)j]; };
        const int fit_slot = slot(s.n_fit);
        for (int k = 0; k < no; ++k) {
            const int i = s.origins[o0 + k];
            org_slot[(size_t)2 * k] = slot(i);
            org_slot[(size_t)2 * k + 1] = slot(i + s.block);
            n_end = std::max(n_end, i + s.block);
        }
        if (s.loglik_out && o0 == 0) n_end = n_rows;             // the pointwise output covers every row, once
        HIP_TRY(hipMemcpyAsync(d_slot_of, slot_of.data(), slot_of.size() * sizeof(int), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_org_slot, org_slot.data(), (size_t)2 * no * sizeof(int), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(d_carry, 0, (size_t)U * sizeof(double), st));
        // stage b + c in blocks of rows, ascending (source 3: one block)
        auto block = [&](long long r0, int nr) -> int {
            ra.row0 = (int)r0;
            acc.nrows = nr;
            HIP_TRY(launch(lfo_accum_kernel, dim3(acc_blocks), dim3(ELPD_THREADS), 0, st, acc));
            return s.loglik_out && o0 == 0 ? pointwise_out(h, s, f, ra, r0, nr) : 0;
        };
        if (int rc = ll_src ? each_block(n_end, n_rows, block) : f.each_rows(h, n_end, block)) return rc;
        // stage d: one work-group per origin of the pass
        LfoRed lr{d_C, ra.cnt, d_org_slot, fit_slot, U, (int)M, S, d_lfo + o0, d_khat + o0, d_tail + o0};
        HIP_TRY(launch(lfo_reduce_kernel, dim3((unsigned)no), dim3(ELPD_THREADS), LFO_LDS_BYTES, st, lr));
        if (int rc = wait_stream(h)) return rc;                  // slot_of and org_slot are rewritten by the next pass
    }
    HIP_TRY(fetch(s.elpd_lfo, d_lfo, (size_t)n_org, st));
    HIP_TRY(fetch(s.khat, d_khat, (size_t)n_org, st));
    HIP_TRY(fetch((long long*)s.tail_len, d_tail, (size_t)n_org, st));
    return wait_stream(h);
}

// ---- recursive forecasts (ptnn_dev_forecast.hpp) ----
int ptnn_forecast(ptnn_handle* h, const ptnn_forecast_spec* spec) {
    // argument checks first: none of them needs the handle or a device
    if (int rc = check_spec(spec, "ptnn_forecast_spec")) return rc;
    const ptnn_forecast_spec& s = *spec;
    const bool host_src = s.w != nullptr, noise = s.noise != 0;
    SampleSource src = source_of(s, host_src, s.eta);
    const RowSource rows{s.origin_source, s.origins, s.n_origins, "origin_source", "PTNN_FORECAST_ORIGIN", "origins", "n_origins"};
    RankOutputs rk{s.n_ranks, s.ranks, s.order_stats};
    if (int rc = check_source(src, "vectors")) return rc;
    if (int rc = check_rows(rows)) return rc;
    if (s.n_origins < 1) return fail(-1, "n_origins = %d must be >= 1", s.n_origins);
    if (s.horizon < 1) return fail(-1, "horizon = %d must be >= 1", s.horizon);
    const long long ncols = (long long)s.n_origins * s.horizon;
    if (ncols > 0x7fffffffLL) return fail(-1, "%d origins x horizon %d = %lld columns: at most 2^31 - 1 per call", s.n_origins, s.horizon, ncols);
    if (int rc = rk.check()) return rc;
    if (noise && host_src && !s.eta) return fail(-1, "noise: host vectors need eta = log tau^2 (one per vector)");
    if (int rc = check_handle(h, "ptnn_forecast")) return rc;
    if (h->cfg.task != PTNN_TASK_REG || h->cfg.n_out != 1)
        return fail(-1, "forecasting needs a regression net with n_out == 1 (a one-step map of one series); this handle is a %s "
                        "net with n_out = %d", h->cfg.task == PTNN_TASK_REG ? "regression" : "classification", h->cfg.n_out);
    const int I = h->cfg.n_in, P = h->P, hz = s.horizon;
    if (int rc = fit_rows(h, rows)) return rc;
    if (int rc = select_samples(h, src, false)) return rc;
    const long long M = src.M;
    if (int rc = rk.check_values(M)) return rc;
    if (s.n_samples) *s.n_samples = M;

    if (int rc = start_device(h)) return rc;
    hipStream_t st = h->stream;
    DeviceScratch mem;
    // origins
    const float* d_x = nullptr;
    int xs = 0;
    if (int rc = upload_rows(h, mem, rows, I, &d_x, &xs)) return rc;
    // stage a: items -> trajectories (noise off: distinct vectors; noise on: every occurrence, host multiplicities expanded)
    std::vector<float> w_exp, eta_exp;
    if (noise) expand_occurrences(src, P, &w_exp, &eta_exp);
    Distinct d;
    if (int rc = distinct_samples(h, mem, src, noise, !noise, &d)) return rc;
    const int U = d.U;
    if (s.n_trajectories) *s.n_trajectories = U;
    // outputs on the device for every column
    double* d_mean = nullptr;
    HIP_TRY(mem.alloc(&d_mean, (size_t)ncols));
    if (int rc = rk.to_device(mem, (size_t)ncols, st)) return rc;
    // stage b + c in blocks of origins and horizon steps: fx 4 U ob hb bytes, + 4 U I bytes of carried windows when the horizon
    // is split (only with one origin per block: the columns of a block are then always contiguous)
    const size_t budget = scratch_budget("PTNN_FORECAST_SCRATCH_BYTES");
    const size_t traj_bytes = (size_t)U * sizeof(float);
    long long ob = 1, hb = hz;
    if (budget >= traj_bytes * hz) {
        ob = std::max(1LL, std::min<long long>((long long)(budget / (traj_bytes * hz)), s.n_origins));
    } else {
        const long long fit = (long long)(budget / traj_bytes) - I;
        hb = std::max(1LL, std::min<long long>(fit, hz));
    }
    ob = std::min<long long>(ob, 65535LL * WAVE);        // grid.y of the split layout
    const bool split_h = hb < hz;
    float *d_fx = nullptr, *d_win = nullptr;
    HIP_TRY(mem.alloc(&d_fx, (size_t)ob * hb * U));
    if (split_h) HIP_TRY(mem.alloc(&d_win, (size_t)U * I));
    ForecastPlan fwd;
    if (int rc = fwd.init(h, d, d_x, xs, hz, d_win, noise, s.seed, d_fx, nullptr)) return rc;
    // samples: the trajectory of every selected row, chain-major
    std::vector<int> item_run;
    if (s.samples) if (int rc = item_runs(h, d, src.n_items, &item_run)) return rc;
    for (long long r0 = 0; r0 < s.n_origins; r0 += ob) {
        const int nr = (int)std::min<long long>(ob, s.n_origins - r0);
        for (long long k0 = 0; k0 < hz; k0 += hb) {
            const int nk = (int)std::min<long long>(hb, hz - k0);
            if (int rc = fwd.run(h, (int)r0, nr, (int)k0, nk)) return rc;
            const long long col0 = r0 * hz + k0;             // the block's columns are contiguous (see above)
            PredictRed ra{d_fx, d.run_cnt, U, 1, (int)col0, (int)ncols, M, s.n_ranks, rk.d_ranks, d_mean, rk.d_stats, nullptr};
            HIP_TRY(launch(predict_reduce_kernel, dim3((unsigned)(nr * nk)), dim3(PRED_THREADS), 0, st, ra));
            if (s.samples)
                if (int rc = scatter_samples(h, d_fx, nr * nk, U, item_run, src.weights(), s.samples, (size_t)ncols, (size_t)col0)) return rc;
        }
    }
    HIP_TRY(fetch(s.mean, d_mean, (size_t)ncols, st));
    HIP_TRY(fetch(s.order_stats, rk.d_stats, (size_t)s.n_ranks * ncols, st));
    return wait_stream(h);
}

// ---- log evidence (ptnn_dev_evidence.hpp) ----
static_assert(PTNN_EVIDENCE_MAX_A == EVID_MAX_A, "ptnn.h prior exponents");

// Stages b and c of the evidence path (ptnn_dev_evidence.hpp), shared by ptnn_evidence and ptnn_mbar: U (and b) of weight vectors
// on the training rows through the per-shape forward pass, and stage e's prior draws through the same two stages.
struct EvidEval {
    ptnn_handle* h = nullptr;
    ForwardPlan fwd;
    const float* d_x = nullptr;                        // training rows
    int xs = 0, I = 0, O = 0, P = 0, N = 0;
    bool reg = false;
    int* d_sse0 = nullptr;                             // weight vectors with SSE = 0 (evid_finish_kernel)
    int init(ptnn_handle* h_, DeviceScratch& mem, const char* what) {
        h = h_;
        I = h->cfg.n_in; O = h->cfg.n_out; P = h->P; N = h->Ntr;
        reg = h->cfg.task == PTNN_TASK_REG;
        if (int rc = fwd.init(h, what)) return rc;
        d_x = h->d_data;
        xs = h->IPY;
        HIP_TRY(mem.alloc(&d_sse0, 1));
        HIP_TRY(hipMemsetAsync(d_sse0, 0, sizeof(int), h->stream));
        return 0;
    }
    // U (and b) of `nv` vectors at base + run_off[u]: rows in blocks of rows_blk, fx scratch `fx` of rows_blk x O x nv floats
    int eval(const float* base, const long long* run_off, int nv, long long rows_blk, float* fx, double* acc, double* u_out, double* b_out) {
        hipStream_t st = h->stream;
        HIP_TRY(hipMemsetAsync(acc, 0, (size_t)nv * sizeof(double), st));
        const unsigned ub = (unsigned)((nv + EVID_THREADS - 1) / EVID_THREADS);
        if (int rc = each_block(N, rows_blk, [&](long long r0, int nr) -> int {
            if (int rc = fwd.run(h, base, run_off, d_x, xs, (int)r0, nr, nv, fx)) return rc;
            EvidRows ra{fx, d_x + (size_t)r0 * xs + I, xs, nr, O, nv, reg ? 1 : 0, acc};
            HIP_TRY(launch(evid_rows_kernel, dim3(ub), dim3(EVID_THREADS), 0, st, ra));
            return 0;
        })) return rc;
        HIP_TRY(launch(evid_finish_kernel, dim3(ub), dim3(EVID_THREADS), 0, st, nv, reg ? 1 : 0, N, acc, u_out, b_out, d_sse0));
        return 0;
    }
    long long rows_for(long long nv, size_t avail) const { return row_block(avail, (size_t)nv * O * sizeof(float), N); }
    int sse_check() {
        int e = 0;
        HIP_TRY(hipMemcpyAsync(&e, d_sse0, sizeof e, hipMemcpyDeviceToHost, h->stream));
        if (int rc = wait_stream(h)) return rc;
        if (e) return fail(-1, "%d weight vectors fit the %d training rows exactly (SSE = 0): U = -(N / 2) log SSE is infinite", e, N);
        return 0;
    }
    // stage e: U and b of prior draws [0, NP) of `seed` into d_pu, d_pb [NP], in blocks of nb vectors (vector + forward scratch of
    // every training row under the budget)
    int prior_draws(DeviceScratch& mem, size_t budget, long long NP, uint64_t seed, double* d_pu, double* d_pb) {
        hipStream_t st = h->stream;
        const size_t per_draw = (size_t)P * sizeof(float) + 4 * sizeof(double) + (size_t)std::min<long long>(N, 65535LL * WAVE) * O * sizeof(float);
        const long long nb = std::max(1LL, std::min<long long>((long long)(budget / per_draw), NP));
        const size_t fixed = (size_t)nb * ((size_t)P * sizeof(float) + 4 * sizeof(double));
        const long long rows_blk = rows_for(nb, budget > fixed ? budget - fixed : 0);
        double* d_acc = nullptr;
        float *d_pw = nullptr, *d_fx = nullptr;
        long long* d_poff = nullptr;
        HIP_TRY(mem.alloc(&d_pw, (size_t)nb * P));
        HIP_TRY(mem.alloc(&d_poff, (size_t)nb));
        HIP_TRY(mem.alloc(&d_acc, (size_t)nb));
        HIP_TRY(mem.alloc(&d_fx, (size_t)rows_blk * O * nb));
        const float sigma = (float)std::sqrt((double)h->cfg.sigma_squared);
        uint32_t slo = 0, shi = 0;
        split_seed(seed, &slo, &shi);
        const int nq = (P + 3) / 4;
        for (long long d0 = 0; d0 < NP; d0 += nb) {
            const int b = (int)std::min<long long>(nb, NP - d0);
            HIP_TRY(launch(evid_prior_kernel, dim3((unsigned)(((long long)b * nq + EVID_THREADS - 1) / EVID_THREADS)), dim3(EVID_THREADS), 0, st,
                           d0, b, P, sigma, slo, shi, d_pw, d_poff));
            if (int rc = eval(d_pw, d_poff, b, rows_blk, d_fx, d_acc, d_pu + d0, d_pb + d0)) return rc;
        }
        return 0;
    }
};

// the split ESS of every rung's U draws (one chain each; rung k's at d_udraw + off[k]), by the convergence kernels: rungs of equal
// length in one pass
static int evid_rung_ess(ptnn_handle* h, const std::vector<long long>& off, const long long* d_off, const double* d_udraw, double* u_ess) {
    hipStream_t st = h->stream;
    const int K = (int)off.size() - 1;
    std::vector<char> done((size_t)K, 0);
    for (int k0 = 0; k0 < K; ++k0) {
        if (done[(size_t)k0]) continue;
        const long long nk = off[(size_t)k0 + 1] - off[(size_t)k0];
        std::vector<int> rung, qcol;
        for (int k = k0; k < K; ++k)
            if (!done[(size_t)k] && off[(size_t)k + 1] - off[(size_t)k] == nk) { rung.push_back(k); done[(size_t)k] = 1; }
        const int Q = (int)rung.size();
        for (int q = 0; q < Q; ++q) qcol.push_back(q);
        DeviceScratch cm;
        int* d_rung = nullptr;
        float* d_draws = nullptr;
        HIP_TRY(cm.alloc(&d_rung, (size_t)Q));
        HIP_TRY(hipMemcpyAsync(d_rung, rung.data(), (size_t)Q * sizeof(int), hipMemcpyHostToDevice, st));
        HIP_TRY(cm.alloc(&d_draws, (size_t)Q * nk));
        HIP_TRY(launch(evid_conv_kernel, dim3((unsigned)(((long long)Q * nk + EVID_THREADS - 1) / EVID_THREADS)), dim3(EVID_THREADS), 0, st,
                       Q, (int)nk, d_off, d_rung, d_udraw, d_draws));
        ConvGather ga{};
        ga.host = 1; ga.draws = d_draws; ga.Qh = Q;
        std::vector<double> ess((size_t)Q);
        if (int rc = conv_drive(h, cm, ga, qcol, 1, (int)nk, 0, nullptr, nullptr, nullptr, ess.data(), nullptr, nullptr, nullptr)) return rc;
        for (int q = 0; q < Q; ++q) u_ess[rung[(size_t)q]] = ess[(size_t)q];
    }
    return 0;
}

// The rungs of ptnn_evidence and ptnn_mbar (Spec: the fields the two specs name alike), from a host U [K][n], host vectors
// [K][n][P] -- one list of K n items, whose [K, n] multiplicities are applied to U -- or the trace, one rung per chain: the expanded
// draws of rung k at [off[k], off[k + 1]), and stages a to c of the evidence path.  In steps, since the order of the refusals is
// kept and each call has checks of its own between them.
extern "C++" {
template <class Spec> struct RungLayout {
    const Spec& s;
    const bool u_src, host_src;
    SampleSource src;
    std::vector<long long> off;                        // [K + 1]
    std::vector<int32_t> item_of;                      // expanded draw -> item (multiplicities only)
    long long per = 0;                                 // rows per rung
    Distinct d;                                        // eval: the distinct vectors
    explicit RungLayout(const Spec& spec)
        : s(spec), u_src(spec.u != nullptr), host_src(spec.w != nullptr),
          src{host_src, spec.w, nullptr, (int64_t)spec.n_rungs * spec.n_per_rung, nullptr, spec.replicas, spec.n_replicas, spec.step0, spec.nsteps, spec.thin} {}
    bool trace() const { return !u_src && !host_src; }
    int K() const { return (int)off.size() - 1; }
    long long n_draws() const { return off.back(); }
    // the host sources, no handle needed: items, their multiplicities, the draws of every rung; not_finite(item, k, i) refuses a
    // counted item whose host U is not finite, in the call's words
    template <class F> int host(F not_finite) {
        if (trace()) return 0;
        const long long K = s.n_rungs, n = per = s.n_per_rung;
        if (K * n > 0x7fffffffLL) return fail(-1, "%lld host rows: at most 2^31 - 1 per call", K * n);
        src.n_items = K * n;
        off.assign((size_t)K + 1, 0);
        for (long long k = 0; k < K; ++k) {
            long long c = 0;
            for (long long i = 0; i < n; ++i) {
                const long long it = k * n + i;
                const int mu = s.multiplicity ? s.multiplicity[it] : 1;
                if (mu < 0) return fail(-1, "multiplicity[%lld, %lld] = %d is negative", k, i, mu);
                c += mu;
                if (s.multiplicity) for (int r = 0; r < mu; ++r) item_of.push_back((int32_t)it);
                if (u_src && mu > 0)
                    if (int rc = not_finite(it, k, i)) return rc;
            }
            off[(size_t)k + 1] = off[(size_t)k] + c;
            if (off[(size_t)k + 1] > 0x7fffffffLL) return fail(-1, "more than 2^31 - 1 expanded draws");
        }
        return 0;
    }
    // the trace selection, with the handle: the rows counted, then -- behind the call's own checks -- one rung per chain
    int count_trace(const ptnn_handle* h) {
        if (int rc = count_samples(h, src)) return rc;
        if (src.n_items > 0x7fffffffLL) return fail(-1, "%lld trace rows: at most 2^31 - 1 per call", src.n_items);
        return 0;
    }
    void trace_rungs() {
        per = src.m;
        off.assign(src.reps.size() + 1, 0);
        for (size_t k = 0; k < src.reps.size(); ++k) off[k + 1] = off[k] + per;
    }
    int four_per_rung() const {
        for (int k = 0; k < K(); ++k)
            if (off[(size_t)k + 1] - off[(size_t)k] < 4)
                return fail(-1, "rung %d holds %lld draws: the split ESS needs at least 4 per rung", k, off[(size_t)k + 1] - off[(size_t)k]);
        return 0;
    }
    // Stages a to c: items -> distinct vectors -> their U (and b, where b_out is given), rows in blocks under the budget -> the U
    // (and b) of n entries at u_out (b_out): the items, or with `d_item_of` the expanded draws
    int eval(ptnn_handle* h, DeviceScratch& mem, EvidEval& ev, size_t budget, long long n, const int* d_item_of, double* u_out, double* b_out) {
        hipStream_t st = h->stream;
        if (int rc = distinct_samples(h, mem, src, false, true, &d)) return rc;
        const int U = d.U;
        if (s.n_distinct) *s.n_distinct = U;
        const long long rows_blk = ev.rows_for(U, budget);
        float* d_fx = nullptr;
        double *d_acc = nullptr, *d_udist = nullptr, *d_bdist = nullptr;
        HIP_TRY(mem.alloc(&d_fx, (size_t)rows_blk * ev.O * U));
        HIP_TRY(mem.alloc(&d_acc, (size_t)U));
        HIP_TRY(mem.alloc(&d_udist, (size_t)U));
        if (b_out) HIP_TRY(mem.alloc(&d_bdist, (size_t)U));
        if (int rc = ev.eval(d.base, d.run_off, U, rows_blk, d_fx, d_acc, d_udist, d_bdist)) return rc;
        const unsigned blocks = (unsigned)((n + EVID_THREADS - 1) / EVID_THREADS);
        HIP_TRY(launch(evid_expand_kernel, dim3(blocks), dim3(EVID_THREADS), 0, st, n, d_item_of, d.item_run, d_udist, u_out));
        if (b_out) HIP_TRY(launch(evid_expand_kernel, dim3(blocks), dim3(EVID_THREADS), 0, st, n, d_item_of, d.item_run, d_bdist, b_out));
        return ev.sse_check();
    }
};
}  // extern "C++"

int ptnn_evidence(ptnn_handle* h, const ptnn_evidence_spec* spec) {
    // argument checks first: none of them needs the handle or a device
    if (int rc = check_spec(spec, "ptnn_evidence_spec")) return rc;
    const ptnn_evidence_spec& s = *spec;
    RungLayout<ptnn_evidence_spec> rungs(s);
    const bool u_src = rungs.u_src, host_src = rungs.host_src;
    SampleSource& src = rungs.src;
    if (u_src && host_src) return fail(-1, "give host vectors w or a host U, not both");
    if (u_src || host_src) {
        if (s.n_rungs < 1) return fail(-1, "n_rungs = %d must be >= 1", s.n_rungs);
        if (s.n_per_rung < 1) return fail(-1, "n_per_rung = %lld must be >= 1", (long long)s.n_per_rung);
    } else {
        if (int rc = check_source(src, "vectors", true, "U")) return rc;
    }
    if (s.n_prior < 0) return fail(-1, "n_prior = %lld must be >= 0", (long long)s.n_prior);
    if (s.n_prior > 0x7fffffffLL) return fail(-1, "n_prior = %lld: at most 2^31 - 1 prior draws per call", (long long)s.n_prior);
    if (s.n_prior > 0 && (s.n_a < 1 || s.n_a > EVID_MAX_A || !s.a))
        return fail(-1, "n_prior = %lld prior draws need 1 to %d exponents a (n_a = %d)", (long long)s.n_prior, EVID_MAX_A, s.n_a);
    if (s.n_prior > 0)
        for (int j = 0; j < s.n_a; ++j)
            if (!std::isfinite(s.a[j])) return fail(-1, "a[%d] = %g is not finite", j, s.a[j]);
    if (s.n_prior == 0 && s.u_prior_out) return fail(-1, "u_prior_out requested with n_prior = 0");
    if (u_src && s.u_out) return fail(-1, "u_out: U is the input of this source");
    if (u_src && s.n_distinct) *s.n_distinct = 0;
    if (int rc = rungs.host([&](long long it, long long k, long long i) {
        return std::isfinite(s.u[it]) ? 0 : fail(-1, "u[%lld, %lld] = %g is not finite", k, i, s.u[it]);
    })) return rc;
    if (int rc = check_handle(h, "ptnn_evidence")) return rc;
    if (rungs.trace()) {
        if (int rc = rungs.count_trace(h)) return rc;
        rungs.trace_rungs();
    }
    const std::vector<long long>& off = rungs.off;
    const long long n_items = src.n_items, n_draws = rungs.n_draws();
    const int K = rungs.K();
    if (int rc = rungs.four_per_rung()) return rc;
    if (s.d)
        for (int k = 0; k < K; ++k)
            if (!std::isfinite(s.d[k])) return fail(-1, "d[%d] = %g is not finite", k, s.d[k]);
    if (s.n_draws)
        for (int k = 0; k < K; ++k) s.n_draws[k] = off[(size_t)k + 1] - off[(size_t)k];

    if (int rc = start_device(h)) return rc;
    hipStream_t st = h->stream;
    DeviceScratch mem;
    const size_t budget = scratch_budget("PTNN_EVIDENCE_SCRATCH_BYTES");
    EvidEval ev;
    if (int rc = ev.init(h, mem, "log evidence")) return rc;

    // ---- the rungs: U of every draw
    double* d_udraw = nullptr;
    if (K > 0) HIP_TRY(mem.alloc(&d_udraw, (size_t)n_draws));
    int* d_item_of = nullptr;
    if (!rungs.item_of.empty()) HIP_TRY(mem.upload(&d_item_of, rungs.item_of.data(), rungs.item_of.size(), st));
    if (u_src) {
        double* d_u = nullptr;
        HIP_TRY(mem.upload(&d_u, s.u, (size_t)n_items, st));
        HIP_TRY(launch(evid_expand_kernel, dim3((unsigned)((n_draws + EVID_THREADS - 1) / EVID_THREADS)), dim3(EVID_THREADS), 0, st, n_draws,
                       d_item_of, nullptr, d_u, d_udraw));
    } else {
        if (int rc = rungs.eval(h, mem, ev, budget, n_draws, d_item_of, d_udraw, nullptr)) return rc;
    }
    // stage d: per-rung moments and stones
    long long* d_off = nullptr;
    double *d_mean = nullptr, *d_var = nullptr, *d_d = nullptr, *d_ls = nullptr, *d_rv = nullptr;
    HIP_TRY(mem.upload(&d_off, off.data(), off.size(), st));
    HIP_TRY(mem.alloc(&d_mean, (size_t)K));
    HIP_TRY(mem.alloc(&d_var, (size_t)K));
    if (s.d) {
        HIP_TRY(mem.upload(&d_d, s.d, (size_t)K, st));
        HIP_TRY(mem.alloc(&d_ls, (size_t)K));
        HIP_TRY(mem.alloc(&d_rv, (size_t)K));
    }
    EvidRung rg{d_udraw, d_off, d_d, d_mean, d_var, d_ls, d_rv};
    HIP_TRY(launch(evid_rung_kernel, dim3((unsigned)K), dim3(EVID_THREADS), 0, st, rg));
    HIP_TRY(fetch(s.u_mean, d_mean, (size_t)K, st));
    HIP_TRY(fetch(s.u_var, d_var, (size_t)K, st));
    HIP_TRY(fetch(s.d ? s.log_stone : nullptr, d_ls, (size_t)K, st));
    HIP_TRY(fetch(s.d ? s.stone_relvar : nullptr, d_rv, (size_t)K, st));
    HIP_TRY(fetch(s.u_out, d_udraw, (size_t)n_draws, st));
    if (int rc = wait_stream(h)) return rc;
    // the split ESS of every rung's U draws (one chain each), by the convergence kernels: rungs of equal length in one pass
    if (s.u_ess)
        if (int rc = evid_rung_ess(h, off, d_off, d_udraw, s.u_ess)) return rc;
    if (s.n_prior == 0) return 0;

    // ---- stage e: prior draws in blocks of nb vectors (vector + forward scratch of every training row under the budget)
    const long long NP = s.n_prior;
    double *d_pu = nullptr, *d_pb = nullptr, *d_a = nullptr;
    HIP_TRY(mem.alloc(&d_pu, (size_t)NP));
    HIP_TRY(mem.alloc(&d_pb, (size_t)NP));
    if (int rc = ev.prior_draws(mem, budget, NP, s.seed, d_pu, d_pb)) return rc;
    HIP_TRY(mem.alloc(&d_a, (size_t)s.n_a));
    HIP_TRY(hipMemcpyAsync(d_a, s.a, (size_t)s.n_a * sizeof(double), hipMemcpyHostToDevice, st));
    double* d_pr = nullptr;
    HIP_TRY(mem.alloc(&d_pr, (size_t)4 * s.n_a));
    EvidPriorRed pr{d_pu, d_pb, NP, d_a, d_pr, d_pr + s.n_a, d_pr + 2 * s.n_a, d_pr + 3 * s.n_a};
    HIP_TRY(launch(evid_prior_reduce_kernel, dim3((unsigned)s.n_a), dim3(EVID_THREADS), 0, st, pr));
    std::vector<double> prh((size_t)4 * s.n_a);
    HIP_TRY(hipMemcpyAsync(prh.data(), d_pr, prh.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(fetch(s.u_prior_out, d_pu, (size_t)NP, st));
    if (int rc = ev.sse_check()) return rc;
    double* outs[4] = {s.prior_log_mean_exp, s.prior_kish_ess, s.prior_u_mean, s.prior_u_var};
    for (int o = 0; o < 4; ++o)
        if (outs[o]) std::copy(prh.begin() + (size_t)o * s.n_a, prh.begin() + (size_t)(o + 1) * s.n_a, outs[o]);
    return 0;
}

// ---- MBAR over every rung (ptnn_dev_mbar.hpp) ----
static_assert(PTNN_MBAR_MAX_STATES == MBAR_MAX_K, "ptnn.h MBAR states");

int ptnn_mbar(ptnn_handle* h, const ptnn_mbar_spec* spec) {
    // argument checks first: none of them needs the handle or a device
    if (int rc = check_spec(spec, "ptnn_mbar_spec")) return rc;
    const ptnn_mbar_spec& s = *spec;
    RungLayout<ptnn_mbar_spec> rungs(s);
    const bool u_src = rungs.u_src, host_src = rungs.host_src;
    SampleSource& src = rungs.src;
    if (u_src && host_src) return fail(-1, "give host vectors w or a host U, not both");
    if (s.b && !u_src) return fail(-1, "b comes with a host U");
    if (s.n_rungs < 1) return fail(-1, "n_rungs = %d must be >= 1", s.n_rungs);
    if (!s.betas) return fail(-1, "betas [n_rungs] is required");
    if (u_src || host_src) {
        if (s.n_per_rung < 1) return fail(-1, "n_per_rung = %lld must be >= 1", (long long)s.n_per_rung);
    } else {
        if (int rc = check_source(src, "vectors", true, "U")) return rc;
        if (s.replicas && s.n_replicas != s.n_rungs) return fail(-1, "n_replicas = %d but n_rungs = %d betas", s.n_replicas, s.n_rungs);
    }
    for (int k = 0; k < s.n_rungs; ++k) {
        if (!std::isfinite(s.betas[k]) || !(s.betas[k] > 0.0)) return fail(-1, "betas[%d] = %g must be finite and > 0", k, s.betas[k]);
        if (k > 0 && !(s.betas[k] > s.betas[k - 1])) return fail(-1, "betas must rise strictly: betas[%d] = %g after %g", k, s.betas[k], s.betas[k - 1]);
    }
    if (s.n_prior < 0) return fail(-1, "n_prior = %lld must be >= 0", (long long)s.n_prior);
    if (s.n_prior > 0x7fffffffLL) return fail(-1, "n_prior = %lld: at most 2^31 - 1 prior draws per call", (long long)s.n_prior);
    if (s.b_prior && !s.u_prior) return fail(-1, "b_prior comes with u_prior");
    if (s.u_prior && s.n_prior < 1) return fail(-1, "u_prior given with n_prior = 0");
    const long long NP = s.n_prior;
    const int K = s.n_rungs + (NP > 0 ? 1 : 0), k0 = NP > 0 ? 1 : 0;
    if (K > MBAR_MAX_K) return fail(-1, "%d states: at most %d per call", K, MBAR_MAX_K);
    if (!std::isfinite(s.target_beta) || s.target_beta < s.betas[0] || s.target_beta > s.betas[s.n_rungs - 1])
        return fail(-1, "target_beta = %g outside the ladder [%g, %g]", s.target_beta, s.betas[0], s.betas[s.n_rungs - 1]);
    if (!(s.tol > 0.0) || !std::isfinite(s.tol)) return fail(-1, "tol = %g must be a finite number > 0", s.tol);
    if (s.max_iter < 1) return fail(-1, "max_iter = %d must be >= 1", s.max_iter);
    if (s.n_resample < 0 || s.n_resample > 0x7fffffffLL) return fail(-1, "n_resample = %lld outside [0, 2^31 - 1]", (long long)s.n_resample);
    if (s.n_resample == 0 && (s.resample_item || s.cum_weight)) return fail(-1, "resample_item and cum_weight need n_resample > 0");
    const bool expect = s.mean || s.var;
    const RowSource xrows = x_rows(s);
    if ((expect || s.resample_w) && (u_src || s.u_prior))
        return fail(-1, "mean, var and resample_w need the items' weight vectors: not with a host U or host prior draws");
    if (s.resample_w && s.n_resample == 0) return fail(-1, "resample_w needs n_resample > 0");
    if (expect) {
        if (s.n_rows < 1) return fail(-1, "n_rows = %d must be >= 1", s.n_rows);
        if (int rc = check_rows(xrows)) return rc;
    }
    for (long long i = 0; s.u_prior && i < NP; ++i)
        if (!std::isfinite(s.u_prior[i]) || (s.b_prior && !std::isfinite(s.b_prior[i]))) return fail(-1, "u_prior / b_prior [%lld] is not finite", i);
    if (u_src && s.n_distinct) *s.n_distinct = 0;
    const int R = s.n_rungs;
    if (int rc = rungs.host([&](long long it, long long k, long long i) {
        return std::isfinite(s.u[it]) && !(s.b && !std::isfinite(s.b[it])) ? 0 : fail(-1, "u / b [%lld, %lld] is not finite", k, i);
    })) return rc;
    if (int rc = check_handle(h, "ptnn_mbar")) return rc;
    const int O = h->cfg.n_out;
    if (expect)
        if (int rc = fit_rows(h, xrows)) return rc;
    if (s.sse && h->cfg.task != PTNN_TASK_REG) return fail(-1, "sse: a classification has no sum of squared errors");
    if (rungs.trace()) {
        if (int rc = rungs.count_trace(h)) return rc;
        if ((int)src.reps.size() != R) return fail(-1, "%d chains selected but n_rungs = %d betas", (int)src.reps.size(), R);
        rungs.trace_rungs();
    }
    if (int rc = rungs.four_per_rung()) return rc;
    const std::vector<long long>& off = rungs.off;
    const std::vector<int32_t>& item_of = rungs.item_of;
    const long long per = rungs.per, n_rows = (long long)R * per, n_draws = rungs.n_draws(), NT = NP + n_rows;
    if (NT > 0x7fffffffLL) return fail(-1, "%lld items: at most 2^31 - 1 per call", NT);
    if (s.n_items) *s.n_items = NT;

    if (int rc = start_device(h)) return rc;
    hipStream_t st = h->stream;
    DeviceScratch mem;
    const size_t budget = scratch_budget("PTNN_EVIDENCE_SCRATCH_BYTES");
    // ---- U and b of every item: the prior draws first, then the rungs' rows
    double *d_u = nullptr, *d_b = nullptr, *d_c = nullptr, *d_D = nullptr;
    HIP_TRY(mem.alloc(&d_u, (size_t)NT));
    HIP_TRY(mem.alloc(&d_b, (size_t)NT));
    HIP_TRY(mem.alloc(&d_c, (size_t)NT));
    HIP_TRY(mem.alloc(&d_D, (size_t)NT));
    HIP_TRY(hipMemsetAsync(d_b, 0, (size_t)NT * sizeof(double), st));
    EvidEval ev;
    const Distinct& d = rungs.d;                       // the rungs' distinct vectors (sources 1, 2)
    const bool need_net = !u_src || (NP > 0 && !s.u_prior);
    if (need_net)
        if (int rc = ev.init(h, mem, "MBAR")) return rc;
    if (u_src) {
        HIP_TRY(hipMemcpyAsync(d_u + NP, s.u, (size_t)n_rows * sizeof(double), hipMemcpyHostToDevice, st));
        if (s.b) HIP_TRY(hipMemcpyAsync(d_b + NP, s.b, (size_t)n_rows * sizeof(double), hipMemcpyHostToDevice, st));
    } else {
        // stages a to c of the evidence path: items -> distinct vectors -> their U and b -> every row's
        if (int rc = rungs.eval(h, mem, ev, budget, n_rows, nullptr, d_u + NP, d_b + NP)) return rc;
    }
    if (s.u_prior) {
        HIP_TRY(hipMemcpyAsync(d_u, s.u_prior, (size_t)NP * sizeof(double), hipMemcpyHostToDevice, st));
        if (s.b_prior) HIP_TRY(hipMemcpyAsync(d_b, s.b_prior, (size_t)NP * sizeof(double), hipMemcpyHostToDevice, st));
    } else if (NP > 0) {
        if (int rc = ev.prior_draws(mem, budget, NP, s.seed, d_u, d_b)) return rc;
        if (int rc = ev.sse_check()) return rc;
    }
    // ---- N_k and c_n: counts, or the split ESS of every rung's expanded U draws (stage d of the evidence path)
    std::vector<double> n_eff((size_t)K, 0.0), scale((size_t)R, 1.0);
    if (NP > 0) n_eff[0] = (double)NP;
    for (int k = 0; k < R; ++k) n_eff[(size_t)(k0 + k)] = (double)(off[(size_t)k + 1] - off[(size_t)k]);
    if (s.effective) {
        long long* d_off = nullptr;
        HIP_TRY(mem.upload(&d_off, off.data(), off.size(), st));
        const double* d_udraw = d_u + NP;
        if (s.multiplicity) {
            int* d_item_of = nullptr;
            double* d_exp = nullptr;
            HIP_TRY(mem.upload(&d_item_of, item_of.data(), item_of.size(), st));
            HIP_TRY(mem.alloc(&d_exp, (size_t)n_draws));
            HIP_TRY(launch(evid_expand_kernel, dim3((unsigned)((n_draws + EVID_THREADS - 1) / EVID_THREADS)), dim3(EVID_THREADS), 0, st, n_draws,
                           d_item_of, nullptr, d_u + NP, d_exp));
            d_udraw = d_exp;
        }
        std::vector<double> ess((size_t)R, 0.0);
        if (int rc = evid_rung_ess(h, off, d_off, d_udraw, ess.data())) return rc;
        for (int k = 0; k < R; ++k) {
            const double e = std::isfinite(ess[(size_t)k]) && ess[(size_t)k] > 0.0 ? ess[(size_t)k] : 1.0;
            scale[(size_t)k] = e / n_eff[(size_t)(k0 + k)];
            n_eff[(size_t)(k0 + k)] = e;
        }
    }
    {
        std::vector<double> c((size_t)NT);
        for (long long i = 0; i < NP; ++i) c[(size_t)i] = 1.0;
        for (long long k = 0; k < R; ++k)
            for (long long i = 0; i < per; ++i)
                c[(size_t)(NP + k * per + i)] = (double)(s.multiplicity ? s.multiplicity[k * per + i] : 1) * scale[(size_t)k];
        HIP_TRY(hipMemcpyAsync(d_c, c.data(), (size_t)NT * sizeof(double), hipMemcpyHostToDevice, st));
        if (int rc = wait_stream(h)) return rc;        // c lives until the copy is done
    }
    // ---- the states and the fixed point
    std::vector<double> hs((size_t)4 * K, 0.0);        // beta, g, ln N, f
    for (int k = 0; k < K; ++k) {
        hs[(size_t)k] = k < k0 ? 0.0 : s.betas[k - k0];
        hs[(size_t)K + k] = k < k0 ? 0.0 : 1.0;
        hs[(size_t)2 * K + k] = std::log(n_eff[(size_t)k]);
    }
    double *d_s = nullptr, *d_raw = nullptr, *d_res = nullptr;
    HIP_TRY(mem.upload(&d_s, hs.data(), hs.size(), st));
    HIP_TRY(mem.alloc(&d_raw, (size_t)K));
    HIP_TRY(mem.alloc(&d_res, 1));
    const MbarItems it{d_u, d_b, d_c, d_D, NT};
    const MbarStates ms{K, d_s, d_s + K, d_s + 2 * K, d_s + 3 * K};
    double* d_f = d_s + 3 * K;
    const unsigned item_blocks = (unsigned)((NT + MBAR_THREADS - 1) / MBAR_THREADS);
    long long n_iter = 0;
    double resid = INFINITY;
    while (n_iter < s.max_iter && !(resid <= s.tol)) {
        for (int q = 0; q < 8; ++q) {
            HIP_TRY(launch(mbar_denominator_kernel, dim3(item_blocks), dim3(MBAR_THREADS), 0, st, it, ms));
            HIP_TRY(launch(mbar_free_energy_kernel, dim3((unsigned)K), dim3(MBAR_THREADS), 0, st, it, ms.beta, ms.g, d_raw));
            HIP_TRY(launch(mbar_pin_kernel, dim3(1), dim3(MBAR_MAX_K), 0, st, K, d_raw, d_f, d_res));
        }
        n_iter += 8;
        HIP_TRY(hipMemcpyAsync(&resid, d_res, sizeof resid, hipMemcpyDeviceToHost, st));
        if (int rc = wait_stream(h)) return rc;
    }
    if (!std::isfinite(resid)) return fail(-2, "the MBAR iteration left the finite numbers after %lld sweeps", n_iter);
    if (s.n_iter) *s.n_iter = n_iter;
    if (s.residual) *s.residual = resid;
    // D of the final f, for W, the Gram matrix and the weights
    HIP_TRY(launch(mbar_denominator_kernel, dim3(item_blocks), dim3(MBAR_THREADS), 0, st, it, ms));
    if (s.n_eff) std::copy(n_eff.begin(), n_eff.end(), s.n_eff);
    HIP_TRY(fetch(s.f, (const double*)d_f, (size_t)K, st));
    HIP_TRY(fetch(s.u_out, (const double*)d_u, (size_t)NT, st));
    HIP_TRY(fetch(s.b_out, (const double*)d_b, (size_t)NT, st));
    if (s.gram) {
        const int nt = (K + MBAR_TILE - 1) / MBAR_TILE, npairs = nt * (nt + 1) / 2;
        const int n_chunks = (int)((NT + MBAR_GRAM_CHUNK - 1) / MBAR_GRAM_CHUNK);
        double *d_part = nullptr, *d_M = nullptr;
        HIP_TRY(mem.alloc(&d_part, (size_t)n_chunks * npairs * MBAR_TILE * MBAR_TILE));
        HIP_TRY(mem.alloc(&d_M, (size_t)K * K));
        const MbarGram ga{it, ms, d_part};
        HIP_TRY(launch(mbar_gram_kernel, dim3((unsigned)((long long)npairs * n_chunks)), dim3(MBAR_THREADS), 0, st, ga));
        HIP_TRY(launch(mbar_gram_sum_kernel, dim3((unsigned)((K * K + MBAR_THREADS - 1) / MBAR_THREADS)), dim3(MBAR_THREADS), 0, st, K, n_chunks,
                       d_part, d_M));
        HIP_TRY(fetch(s.gram, (const double*)d_M, (size_t)K * K, st));
    }
    // ---- the weights at the target beta, their statistics, systematic resampling
    double *d_t = nullptr, *d_lw = nullptr, *d_ws = nullptr;
    const double tgt[3] = {s.target_beta, 1.0, 0.0};   // beta, g, its free energy
    HIP_TRY(mem.upload(&d_t, tgt, 3, st));
    HIP_TRY(mem.alloc(&d_lw, (size_t)NT));
    HIP_TRY(mem.alloc(&d_ws, 4));
    HIP_TRY(launch(mbar_free_energy_kernel, dim3(1), dim3(MBAR_THREADS), 0, st, it, d_t, d_t + 1, d_t + 2));
    HIP_TRY(launch(mbar_weight_kernel, dim3(item_blocks), dim3(MBAR_THREADS), 0, st, it, d_t, d_t + 2, d_lw));
    HIP_TRY(launch(mbar_weight_stats_kernel, dim3(1), dim3(MBAR_THREADS), 0, st, d_lw, d_c, NT, d_ws));
    HIP_TRY(fetch(s.log_weight, (const double*)d_lw, (size_t)NT, st));
    double ws[4] = {0, 0, 0, 0};
    if (s.n_resample > 0) {
        double* d_cum = nullptr;
        long long* d_item = nullptr;
        uint32_t slo = 0, shi = 0;
        split_seed(s.resample_seed, &slo, &shi);
        HIP_TRY(mem.alloc(&d_cum, (size_t)NT));
        HIP_TRY(mem.alloc(&d_item, (size_t)s.n_resample));
        HIP_TRY(launch(mbar_scan_kernel, dim3(1), dim3(MBAR_THREADS), 0, st, d_lw, NT, d_cum));
        HIP_TRY(launch(mbar_resample_kernel, dim3((unsigned)((s.n_resample + MBAR_THREADS - 1) / MBAR_THREADS)), dim3(MBAR_THREADS), 0, st, d_cum,
                       NT, (long long)s.n_resample, slo, shi, d_item, d_ws + 3));
        HIP_TRY(fetch(s.cum_weight, (const double*)d_cum, (size_t)NT, st));
        static_assert(sizeof(long long) == sizeof(int64_t), "resample_item");
        HIP_TRY(fetch(reinterpret_cast<long long*>(s.resample_item), (const long long*)d_item, (size_t)s.n_resample, st));
        if (s.resample_w) {
            float* d_rw = nullptr;
            const int P = h->P;
            HIP_TRY(mem.alloc(&d_rw, (size_t)s.n_resample * P));
            uint32_t plo = 0, phi = 0;
            split_seed(s.seed, &plo, &phi);
            const MbarGather ga{d_item, (long long)s.n_resample, NP, P, (float)std::sqrt((double)h->cfg.sigma_squared), plo, phi, d.base, d.run_off,
                                d.item_run, d_rw};
            const long long nth = (long long)s.n_resample * ((P + 3) / 4);
            HIP_TRY(launch(mbar_gather_kernel, dim3((unsigned)((nth + MBAR_THREADS - 1) / MBAR_THREADS)), dim3(MBAR_THREADS), 0, st, ga));
            HIP_TRY(fetch(s.resample_w, (const float*)d_rw, (size_t)s.n_resample * P, st));
        }
    }
    // ---- expectations of the network outputs on the rows x under the target weights (mbar_expect_kernel)
    if (expect) {
        const int I = h->cfg.n_in, P = h->P, n_x = s.n_rows, ncols = n_x * O, U = d.U;
        const float* d_x = nullptr;
        int xs = 0;
        if (int rc = upload_rows(h, mem, xrows, I, &d_x, &xs)) return rc;
        double *d_acc = nullptr, *d_mean = nullptr, *d_var = nullptr;
        HIP_TRY(mem.alloc(&d_acc, (size_t)ncols));
        HIP_TRY(mem.alloc(&d_mean, (size_t)ncols));
        HIP_TRY(mem.alloc(&d_var, (size_t)ncols));
        // the rungs' distinct vectors on blocks of rows; prior draws in blocks of nb vectors, a multiple of the kernel's chunk
        const long long rblk = row_block(budget, (size_t)U * O * sizeof(float), n_x);
        float *d_fx = nullptr, *d_pw = nullptr, *d_pfx = nullptr;
        long long* d_poff = nullptr;
        HIP_TRY(mem.alloc(&d_fx, (size_t)rblk * O * U));
        long long nb = 0, pblk = 0;
        if (NP > 0) {
            const size_t per_draw = (size_t)P * sizeof(float) + sizeof(long long) + (size_t)WAVE * O * sizeof(float);
            nb = std::min<long long>(NP, std::max<long long>(MBAR_THREADS, (long long)(budget / per_draw) / MBAR_THREADS * MBAR_THREADS));
            const size_t fixed = (size_t)nb * ((size_t)P * sizeof(float) + sizeof(long long));
            pblk = row_block(budget > fixed ? budget - fixed : 0, (size_t)nb * O * sizeof(float), n_x);
            HIP_TRY(mem.alloc(&d_pw, (size_t)nb * P));
            HIP_TRY(mem.alloc(&d_poff, (size_t)nb));
            HIP_TRY(mem.alloc(&d_pfx, (size_t)pblk * O * nb));
        }
        const float sigma = (float)std::sqrt((double)h->cfg.sigma_squared);
        uint32_t slo = 0, shi = 0;
        split_seed(s.seed, &slo, &shi);
        const int nq = (P + 3) / 4;
        auto pass = [&](const double* mean) -> int {
            HIP_TRY(hipMemsetAsync(d_acc, 0, (size_t)ncols * sizeof(double), st));
            if (int rc = each_block(n_x, rblk, [&](long long r0, int nr) -> int {
                if (int rc = ev.fwd.run(h, d.base, d.run_off, d_x, xs, (int)r0, nr, U, d_fx)) return rc;
                const MbarExpect ea{d_fx, U, d.item_run, d_lw + NP, n_rows, mean, d_acc, (int)r0 * O};
                HIP_TRY(launch(mbar_expect_kernel, dim3((unsigned)(nr * O)), dim3(MBAR_THREADS), 0, st, ea));
                return 0;
            })) return rc;
            for (long long d0 = 0; d0 < NP; d0 += nb) {
                const int b = (int)std::min<long long>(nb, NP - d0);
                HIP_TRY(launch(evid_prior_kernel, dim3((unsigned)(((long long)b * nq + EVID_THREADS - 1) / EVID_THREADS)), dim3(EVID_THREADS), 0, st,
                               d0, b, P, sigma, slo, shi, d_pw, d_poff));
                if (int rc = each_block(n_x, pblk, [&](long long r0, int nr) -> int {
                    if (int rc = ev.fwd.run(h, d_pw, d_poff, d_x, xs, (int)r0, nr, b, d_pfx)) return rc;
                    const MbarExpect ea{d_pfx, b, nullptr, d_lw + d0, (long long)b, mean, d_acc, (int)r0 * O};
                    HIP_TRY(launch(mbar_expect_kernel, dim3((unsigned)(nr * O)), dim3(MBAR_THREADS), 0, st, ea));
                    return 0;
                })) return rc;
            }
            return 0;
        };
        const unsigned cb = (unsigned)((ncols + MBAR_THREADS - 1) / MBAR_THREADS);
        if (int rc = pass(nullptr)) return rc;
        HIP_TRY(launch(mbar_expect_finish_kernel, dim3(cb), dim3(MBAR_THREADS), 0, st, ncols, d_acc, d_ws, d_mean));
        if (s.var) {
            if (int rc = pass(d_mean)) return rc;
            HIP_TRY(launch(mbar_expect_finish_kernel, dim3(cb), dim3(MBAR_THREADS), 0, st, ncols, d_acc, d_ws, d_var));
        }
        HIP_TRY(fetch(s.mean, (const double*)d_mean, (size_t)ncols, st));
        HIP_TRY(fetch(s.var, (const double*)d_var, (size_t)ncols, st));
    }
    HIP_TRY(fetch(s.sse, (const double*)d_b, (size_t)NT, st));       // b = -log SSE; finished below
    HIP_TRY(hipMemcpyAsync(ws, d_ws, sizeof ws, hipMemcpyDeviceToHost, st));
    if (int rc = wait_stream(h)) return rc;
    for (long long n = 0; s.sse && n < NT; ++n) s.sse[n] = std::exp(-s.sse[n]);
    // the map of the items: prior draws, then every rung's rows
    const bool trace = !u_src && !host_src;
    for (long long n = 0; n < NT && (s.item_chain || s.item_step || s.item_multiplicity); ++n) {
        const long long r = n - NP, k = r < 0 ? -1 : r / per, i = r < 0 ? n : r % per;
        if (s.item_chain) s.item_chain[n] = r < 0 ? -1 : trace ? src.reps[(size_t)k] : (int32_t)k;
        if (s.item_step) s.item_step[n] = r >= 0 && trace ? (int64_t)s.step0 + i * s.thin : i;
        if (s.item_multiplicity) s.item_multiplicity[n] = r >= 0 && s.multiplicity ? s.multiplicity[r] : 1;
    }
    if (s.weight_sum) *s.weight_sum = ws[0];
    if (s.kish_ess) *s.kish_ess = ws[1];
    if (s.max_weight_share) *s.max_weight_share = ws[2];
    if (s.resample_u) *s.resample_u = s.n_resample > 0 ? ws[3] : 0.0;
    return 0;
}

// ---- calibration (ptnn_dev_calibration.hpp) ----
static_assert(PTNN_CALIB_MAX_LEVELS == CALIB_MAX_LEVELS && PTNN_CALIB_MAX_DISTINCT == CALIB_MAX_DISTINCT, "ptnn.h calibration limits");

int ptnn_calibration(ptnn_handle* h, const ptnn_calibration_spec* spec) {
    // argument checks first: none of them needs the handle or a device
    if (int rc = check_spec(spec, "ptnn_calibration_spec")) return rc;
    const ptnn_calibration_spec& s = *spec;
    RowsByVectors f(s, x_rows(s), s.w != nullptr);
    if (int rc = f.check_source()) return rc;
    if (s.n_rows < 1) return fail(-1, "n_rows = %d must be >= 1", s.n_rows);
    if (int rc = check_rows(f.rows)) return rc;
    if (int rc = MixtureColumns<ptnn_calibration_spec>::check(s)) return rc;
    if (int rc = f.count_host()) return rc;
    if (int rc = check_handle(h, "ptnn_calibration")) return rc;
    const int I = h->cfg.n_in, O = h->cfg.n_out;
    const bool reg = h->cfg.task == PTNN_TASK_REG;
    const bool reg_out = s.pit || s.crps || s.pred_mean || s.pred_sd || s.quantiles || s.pair_term;
    if (reg_out && (!reg || O != 1))
        return fail(-1, "pit, crps, pred_mean, pred_sd and quantiles need a regression net with n_out == 1; this handle is a %s net "
                        "with n_out = %d", reg ? "regression" : "classification", O);
    if (s.p_mean && reg) return fail(-1, "p_mean: a regression has no class probabilities");
    if (int rc = f.fit(h)) return rc;
    if (int rc = f.select(h, s.n_samples)) return rc;

    // stage a: items -> distinct (w, eta) samples (a classification's: distinct w, as ptnn_predict's)
    f.eta = reg;
    if (int rc = f.stage(h, I + 1, s.n_distinct)) return rc;
    hipStream_t st = h->stream;
    const int n_rows = s.n_rows, U = f.U;
    if (s.pair_term && U > CALIB_MAX_DISTINCT)
        return fail(-1, "%d distinct samples: the pair term of the CRPS takes at most %d (U^2 / 2 terms per data row); select fewer "
                        "samples (thin=, chains=) or leave the CRPS out (crps=False)", U, CALIB_MAX_DISTINCT);
    if (int rc = f.forward(h, "PTNN_CALIB_SCRATCH_BYTES", 1, (size_t)U * sizeof(float) * O, n_rows, "calibration")) return rc;

    if (!reg) {
        double* d_mean = nullptr;
        HIP_TRY(f.mem.alloc(&d_mean, (size_t)n_rows * O));
        if (int rc = f.each_rows(h, n_rows, [&](long long r0, int nr) -> int {
            PredictRed ra{f.d_fx, f.d.run_cnt, U, O, (int)r0 * O, n_rows * O, f.M, 0, nullptr, d_mean, nullptr, nullptr};
            HIP_TRY(launch(predict_reduce_kernel, dim3((unsigned)(nr * O)), dim3(PRED_THREADS), 0, st, ra));
            return 0;
        })) return rc;
        HIP_TRY(fetch(s.p_mean, d_mean, (size_t)n_rows * O, st));
        return wait_stream(h);
    }

    MixtureColumns<ptnn_calibration_spec> mc{h, f, s, n_rows, false};
    if (int rc = mc.alloc(f.d_fx, f.d_x + I, f.xs)) return rc;
    if (int rc = f.each_rows(h, n_rows, [&](long long r0, int nr) { return mc.block(r0, nr); })) return rc;
    if (int rc = mc.finish()) return rc;
    if (int rc = mc.fetch()) return rc;
    return wait_stream(h);
}

// ---- forecast verification (ptnn_dev_fscore.hpp) ----
int ptnn_forecast_score(ptnn_handle* h, const ptnn_forecast_score_spec* spec) {
    // argument checks first: none of them needs the handle or a device
    if (int rc = check_spec(spec, "ptnn_forecast_score_spec")) return rc;
    const ptnn_forecast_score_spec& s = *spec;
    const bool host_src = s.w != nullptr, noise = s.noise != 0, pair = s.pair_term != 0, energy = s.energy != 0;
    RowsByVectors f(s, RowSource{s.origin_source, s.origins, s.n_origins, "origin_source", "PTNN_FORECAST_ORIGIN", "origins", "n_origins"},
                    host_src);
    SampleSource& src = f.src;
    if (int rc = check_source(src, "vectors")) return rc;      // (an empty trace selection is refused with the handle)
    if (int rc = check_rows(f.rows)) return rc;
    if (s.n_origins < 1) return fail(-1, "n_origins = %d must be >= 1", s.n_origins);
    if (s.horizon < 1) return fail(-1, "horizon = %d must be >= 1", s.horizon);
    const long long ncols = (long long)s.n_origins * s.horizon;
    if (ncols > 0x7fffffffLL) return fail(-1, "%d origins x horizon %d = %lld columns: at most 2^31 - 1 per call", s.n_origins, s.horizon, ncols);
    if (!s.truth) return fail(-1, "truth is NULL: forecast verification needs the observed values [n_origins, horizon] (NaN = none)");
    const int hz = s.horizon, n_org = s.n_origins;
    // the steps with truth of every origin
    std::vector<int> klist((size_t)ncols, 0), nk((size_t)n_org, 0);
    long long n_finite = 0;
    for (long long c = 0; c < ncols; ++c) {
        const float v = s.truth[c];
        if (std::isinf(v)) return fail(-1, "truth[%lld, %lld] = %g is infinite: NaN marks a missing observation", c / hz, c % hz, (double)v);
        if (v == v) { const size_t r = (size_t)(c / hz); klist[r * hz + nk[r]++] = (int)(c % hz); ++n_finite; }
    }
    if (n_finite == 0) return fail(-1, "truth holds no finite entry: nothing to score");
    if (int rc = MixtureColumns<ptnn_forecast_score_spec>::check(s)) return rc;
    if (s.energy_score && !energy) return fail(-1, "energy_score requested without energy");
    if (energy && hz > PTNN_FSCORE_MAX_ENERGY_HORIZON)
        return fail(-1, "energy: horizon = %d, the energy score takes paths of at most %d steps (energy=False)", hz, PTNN_FSCORE_MAX_ENERGY_HORIZON);
    if (noise && host_src && !s.eta) return fail(-1, "noise: host vectors need eta = log tau^2 (one per vector)");
    if (int rc = f.count_host()) return rc;
    if (int rc = check_handle(h, "ptnn_forecast_score")) return rc;
    if (h->cfg.task != PTNN_TASK_REG || h->cfg.n_out != 1)
        return fail(-1, "forecast verification needs a regression net with n_out == 1 (a one-step map of one series); this handle is a "
                        "%s net with n_out = %d", h->cfg.task == PTNN_TASK_REG ? "regression" : "classification", h->cfg.n_out);
    const int I = h->cfg.n_in, P = h->P;
    if (int rc = f.fit(h)) return rc;
    if (int rc = f.select(h, s.n_samples)) return rc;
    const long long M = f.M;
    const char* cap_text = "%lld trajectories: the pair term of the CRPS and the energy score take at most %d (U^2 / 2 terms per column or "
                           "origin); select fewer samples (thin=, chains=) or leave them out (crps=False, energy=False)";
    if ((pair || energy) && noise && M > CALIB_MAX_DISTINCT) return fail(-1, cap_text, M, CALIB_MAX_DISTINCT);

    // stage a, as ptnn_forecast: noise on -- every occurrence its own trajectory, host multiplicities expanded; noise off -- the
    // distinct (w, eta) samples with their multiplicities
    std::vector<float> w_exp, eta_exp;
    f.eta = true; f.merge = !noise;
    if (int rc = f.stage(h, I, s.n_trajectories, [&] { if (noise) expand_occurrences(src, P, &w_exp, &eta_exp); return 0; })) return rc;
    hipStream_t st = h->stream;
    DeviceScratch& mem = f.mem;
    const Distinct& d = f.d;
    const int U = f.U;
    if ((pair || energy) && U > CALIB_MAX_DISTINCT) return fail(-1, cap_text, (long long)U, CALIB_MAX_DISTINCT);
    // blocks: 4 U bytes per column for the paths, as much again for mu when the noise makes them differ.  With the energy score a
    // block is whole origins; else origins and horizon steps as ptnn_forecast blocks them (the windows carried)
    const size_t budget = scratch_budget("PTNN_FSCORE_SCRATCH_BYTES");
    const size_t col_bytes = (size_t)U * sizeof(float) * (noise ? 2 : 1);
    long long ob = 1, hb = hz;
    if (budget >= col_bytes * hz) {
        ob = std::max(1LL, std::min<long long>((long long)(budget / (col_bytes * hz)), n_org));
    } else {
        if (energy)
            return fail(-1, "energy: one origin's %d steps of %d trajectories need %zu bytes of scratch, PTNN_FSCORE_SCRATCH_BYTES allows %zu "
                            "(energy=False scores the steps in blocks)", hz, U, col_bytes * hz, budget);
        const long long fit = (long long)(budget / col_bytes) - I;
        hb = std::max(1LL, std::min<long long>(fit, hz));
    }
    hb = std::min<long long>(hb, 65535LL);                                  // a block's columns are grid.y of calib_pair_kernel
    ob = std::min<long long>({ob, 65535LL * WAVE, std::max(1LL, 65535LL / hb)});
    const bool split_h = hb < hz;
    float *d_fx = nullptr, *d_mu = nullptr, *d_win = nullptr, *d_truth = nullptr;
    HIP_TRY(mem.alloc(&d_fx, (size_t)ob * hb * U));
    if (noise) HIP_TRY(mem.alloc(&d_mu, (size_t)ob * hb * U));
    if (split_h) HIP_TRY(mem.alloc(&d_win, (size_t)U * I));
    HIP_TRY(mem.upload(&d_truth, s.truth, (size_t)ncols, st));
    ForecastPlan fwd;
    if (int rc = fwd.init(h, d, f.d_x, f.xs, hz, d_win, noise, s.seed, d_fx, d_mu)) return rc;
    if (int rc = f.items(h, s.samples || s.means)) return rc;
    // per-column and per-origin results: NaN (all bits set) wherever nothing is scored.  The mixture's columns read mu of the
    // block's columns; the log score and the energy score are this call's own
    const float* d_m = noise ? d_mu : d_fx;
    MixtureColumns<ptnn_forecast_score_spec> mc{h, f, s, ncols, true};
    if (int rc = mc.alloc(d_m, d_truth, 1)) return rc;
    double *d_log = nullptr, *d_es = nullptr, *d_et1 = nullptr, *d_eb = nullptr;
    unsigned long long* d_elimbs = nullptr;
    int *d_klist = nullptr, *d_nk = nullptr;
    HIP_TRY(mc.column(&d_log, (size_t)ncols));
    const int n_tiles = mc.n_tiles;
    const unsigned n_tri = mc.n_tri;
    FscoreEnergy ea{};
    size_t e_lds = 0;
    if (energy) {
        HIP_TRY(mc.column(&d_es, (size_t)n_org));
        HIP_TRY(mc.column(&d_et1, (size_t)n_org));
        HIP_TRY(mc.column(&d_eb, (size_t)n_org));
        HIP_TRY(mem.alloc(&d_elimbs, (size_t)n_org * 4));
        HIP_TRY(hipMemsetAsync(d_elimbs, 0, (size_t)n_org * 4 * sizeof(unsigned long long), st));
        HIP_TRY(mem.upload(&d_klist, klist.data(), klist.size(), st));
        HIP_TRY(mem.upload(&d_nk, nk.data(), nk.size(), st));
        int JW = FSCORE_THREADS;                        // the j-paths staged at a time: all steps of JW paths within FSCORE_ENERGY_LDS
        while (JW > FSCORE_JGROUP && (size_t)JW * hz * sizeof(float) > (size_t)FSCORE_ENERGY_LDS) JW >>= 1;
        e_lds = (size_t)JW * hz * sizeof(float);
        if (int rc = raise_lds_limit(reinterpret_cast<const void*>(fscore_energy_kernel), e_lds)) return rc;
        ea.fx = d_fx; ea.cnt = d.run_cnt; ea.y = d_truth; ea.klist = d_klist; ea.nk = d_nk; ea.U = U; ea.hz = hz; ea.S = M;
        ea.term1 = d_et1; ea.bound = d_eb; ea.n_tiles = n_tiles; ea.JW = JW; ea.limbs = d_elimbs;
    }
    FscoreLog la{d_m, d.run_eta, d.run_cnt, d_truth, U, 0, M, d_log};
    for (long long r0 = 0; r0 < n_org; r0 += ob) {
        const int nr = (int)std::min<long long>(ob, n_org - r0);
        for (long long k0 = 0; k0 < hz; k0 += hb) {
            const int nk_blk = (int)std::min<long long>(hb, hz - k0);
            if (int rc = fwd.run(h, (int)r0, nr, (int)k0, nk_blk)) return rc;
            const long long col0 = r0 * hz + k0;             // the block's columns are contiguous (split_h: one origin per block)
            const int nc = nr * nk_blk;                      // <= 65535
            if (int rc = mc.block(col0, nc)) return rc;
            la.col0 = (int)col0;
            HIP_TRY(launch(fscore_logscore_kernel, dim3((unsigned)nc), dim3(FSCORE_THREADS), 0, st, la));
            if (energy) {                                    // hb == hz: whole origins
                ea.r0 = (int)r0;
                HIP_TRY(launch(fscore_energy_first_kernel, dim3((unsigned)nr), dim3(FSCORE_THREADS), 0, st, ea));
                HIP_TRY(launch(fscore_energy_kernel, dim3(n_tri, (unsigned)nr), dim3(FSCORE_THREADS), e_lds, st, ea));
            }
            if (s.samples)
                if (int rc = scatter_samples(h, d_fx, nc, U, f.item_run, src.weights(), s.samples, (size_t)ncols, (size_t)col0)) return rc;
            if (s.means)
                if (int rc = scatter_samples(h, d_m, nc, U, f.item_run, src.weights(), s.means, (size_t)ncols, (size_t)col0)) return rc;
        }
    }
    if (int rc = mc.finish()) return rc;
    if (energy)
        HIP_TRY(launch(fscore_energy_finish_kernel, dim3((unsigned)((n_org + FSCORE_THREADS - 1) / FSCORE_THREADS)), dim3(FSCORE_THREADS), 0, st,
                       n_org, d_nk, d_elimbs, d_et1, d_eb, M, d_es));
    if (int rc = mc.fetch()) return rc;
    HIP_TRY(fetch(s.log_score, d_log, (size_t)ncols, st));
    HIP_TRY(fetch(s.energy_score, d_es, (size_t)n_org, st));
    return wait_stream(h);
}

// ---- posterior predictive checks (ptnn_dev_ppc.hpp) ----
static_assert(PTNN_PPC_MAX_LAGS == PPC_MAX_LAGS, "ptnn.h ppc limits");

int ptnn_ppc(ptnn_handle* h, const ptnn_ppc_spec* spec) {
    // argument checks first: none of them needs the handle or a device
    if (int rc = check_spec(spec, "ptnn_ppc_spec")) return rc;
    const ptnn_ppc_spec& s = *spec;
    RowsByVectors f(s, x_rows(s), s.w != nullptr);
    if (int rc = f.check_source()) return rc;
    if (s.n_rows < 2) return fail(-1, "n_rows = %d: a posterior predictive check needs at least 2 data rows", s.n_rows);
    if (int rc = check_rows(f.rows)) return rc;
    if (s.n_lags < 0 || s.n_lags > PPC_MAX_LAGS) return fail(-1, "n_lags = %d outside [0, %d]", s.n_lags, PPC_MAX_LAGS);
    if (s.n_lags > 0 && !s.lags) return fail(-1, "n_lags = %d but lags is NULL", s.n_lags);
    for (int k = 0; k < s.n_lags; ++k) {
        if (s.lags[k] < 1 || s.lags[k] > s.n_rows - 1)
            return fail(-1, "lags[%d] = %d outside [1, n_rows - 1 = %d]", k, s.lags[k], s.n_rows - 1);
        for (int j = 0; j < k; ++j)
            if (s.lags[j] == s.lags[k]) return fail(-1, "lags[%d] = lags[%d] = %d: a lag may be listed once", j, k, s.lags[k]);
    }
    if (int rc = f.count_host()) return rc;
    if (int rc = check_handle(h, "ptnn_ppc")) return rc;
    const int I = h->cfg.n_in, O = h->cfg.n_out;
    const bool reg = h->cfg.task == PTNN_TASK_REG;
    if (reg && O != 1) return fail(-1, "a regression's posterior predictive check needs n_out == 1; this handle has n_out = %d", O);
    if (!reg && s.n_lags > 0) return fail(-1, "lags: a classification has no residual autocorrelation");
    if (!reg && s.z) return fail(-1, "z: a classification draws classes, not normal deviates");
    if (reg && s.y_rep) return fail(-1, "y_rep: a regression's replicate is f + tau z; request z");
    if (int rc = f.fit(h)) return rc;
    if (int rc = f.select(h, nullptr)) return rc;
    const long long M = f.M;
    const int N = s.n_rows;
    const int n_stats = reg ? PPC_REG_FIXED + s.n_lags : PPC_CLS_FIXED + O;
    // a wave keeps its series in LDS: N doubles (regression), one counter per class (classification)
    const size_t wave_doubles = reg ? (size_t)N : (size_t)(O + 1) / 2;
    if (wave_doubles * sizeof(double) > LDS_CEILING)
        return fail(-1, "n_rows = %d: the residual series of a posterior predictive check is kept in LDS, at most %d rows", N,
                    (int)(LDS_CEILING / sizeof(double)));
    if ((long long)N > 65535LL * WAVE) return fail(-1, "n_rows = %d: at most %lld rows per call", N, 65535LL * WAVE);
    if (s.n_samples) *s.n_samples = M;

    // stage a: items -> distinct (w, eta) samples (a classification's: distinct w, as ptnn_predict's)
    f.eta = reg;
    if (int rc = f.stage(h, I + 1, s.n_distinct)) return rc;
    hipStream_t st = h->stream;
    DeviceScratch& mem = f.mem;
    const Distinct& d = f.d;
    const std::vector<int>& item_run = f.item_run;
    const int U = f.U;
    // the distinct vector of every occurrence, chain-major with the multiplicities expanded: non-decreasing
    if (int rc = f.items(h, true)) return rc;
    if (int rc = wait_stream(h)) return rc;
    std::vector<int> occ_u;
    occ_u.reserve((size_t)M);
    const int32_t* mult = f.src.weights();
    for (size_t k = 0; k < item_run.size(); ++k) {
        if (item_run[k] < 0 || item_run[k] >= U || (!occ_u.empty() && item_run[k] < occ_u.back()))
            return fail(-2, "run-length pass: item %lld belongs to run %d of %d (internal error)", (long long)k, item_run[k], U);
        occ_u.insert(occ_u.end(), (size_t)(mult ? mult[k] : 1), item_run[k]);
    }
    if ((long long)occ_u.size() != M) return fail(-2, "%lld occurrences expanded, %lld counted (internal error)", (long long)occ_u.size(), M);
    int* d_occ = nullptr;
    HIP_TRY(mem.upload(&d_occ, occ_u.data(), (size_t)M, st));

    double *d_tobs = nullptr, *d_trep = nullptr;
    float* d_z = nullptr;
    int* d_yrep = nullptr;
    HIP_TRY(mem.alloc(&d_tobs, (size_t)U * n_stats));
    HIP_TRY(mem.alloc(&d_trep, (size_t)M * n_stats));
    if (s.z) HIP_TRY(mem.alloc(&d_z, (size_t)M * N));
    if (s.y_rep) HIP_TRY(mem.alloc(&d_yrep, (size_t)M * N));
    // blocks of distinct vectors, every one with all rows: fx scratch nu x (rows x O) floats under the budget
    const long long vec_blk = std::max(1LL, std::min<long long>((long long)(scratch_budget("PTNN_PPC_SCRATCH_BYTES") /
                                                                            ((size_t)N * O * sizeof(float))), U));
    float* d_fx = nullptr;
    HIP_TRY(mem.alloc(&d_fx, (size_t)vec_blk * N * O));
    const ForwardPlan& fwd = f.fwd;
    if (int rc = f.fwd.init(h, "posterior predictive check")) return rc;
    const int waves = (int)std::max<size_t>(1, std::min<size_t>(PPC_THREADS / WAVE, (64 * 1024) / (wave_doubles * sizeof(double))));
    const size_t lds = (size_t)waves * wave_doubles * sizeof(double);
    const auto kernel = reg ? ppc_occurrence_kernel<true> : ppc_occurrence_kernel<false>;
    if (int rc = raise_lds_limit(reinterpret_cast<const void*>(kernel), lds)) return rc;
    PpcJob ja{};
    ja.n_rows = N; ja.O = O; ja.fx = d_fx; ja.eta = d.run_eta; ja.y = f.d_x + I; ja.ys = f.xs;
    ja.n_lags = s.n_lags;
    for (int k = 0; k < s.n_lags; ++k) ja.lags[k] = s.lags[k];
    split_seed(s.seed, &ja.seed_lo, &ja.seed_hi);
    ja.occ_u = d_occ; ja.n_stats = n_stats; ja.wave_doubles = (int)wave_doubles;
    ja.t_obs = d_tobs; ja.t_rep = d_trep; ja.z = d_z; ja.y_rep = d_yrep;
    for (long long u0 = 0; u0 < U; u0 += vec_blk) {
        const int nu = (int)std::min<long long>(vec_blk, U - u0);
        if (int rc = fwd.run(h, d.base, d.run_off + u0, f.d_x, f.xs, 0, N, nu, d_fx)) return rc;
        const long long i0 = std::lower_bound(occ_u.begin(), occ_u.end(), (int)u0) - occ_u.begin();
        const long long i1 = std::lower_bound(occ_u.begin(), occ_u.end(), (int)(u0 + nu)) - occ_u.begin();
        ja.nu = nu; ja.u0 = (int)u0; ja.i0 = i0; ja.n_occ = (int)(i1 - i0);
        const long long jobs = (long long)nu + (i1 - i0);
        HIP_TRY(launch(kernel, dim3((unsigned)((jobs + waves - 1) / waves)), dim3((unsigned)(waves * WAVE)), lds, st, ja));
    }
    long long *d_nd = nullptr, *d_ng = nullptr, *d_ne = nullptr;
    double *d_mo = nullptr, *d_mr = nullptr, *d_vr = nullptr;
    HIP_TRY(mem.alloc(&d_nd, (size_t)n_stats));
    HIP_TRY(mem.alloc(&d_ng, (size_t)n_stats));
    HIP_TRY(mem.alloc(&d_ne, (size_t)n_stats));
    HIP_TRY(mem.alloc(&d_mo, (size_t)n_stats));
    HIP_TRY(mem.alloc(&d_mr, (size_t)n_stats));
    HIP_TRY(mem.alloc(&d_vr, (size_t)n_stats));
    PpcReduce ra{M, n_stats, d_occ, d_tobs, d_trep, d_nd, d_ng, d_ne, d_mo, d_mr, d_vr};
    HIP_TRY(launch(ppc_reduce_kernel, dim3((unsigned)n_stats), dim3(PPC_THREADS), 0, st, ra));
    std::vector<double> tobs_h(s.t_obs ? (size_t)U * n_stats : 0);
    HIP_TRY(fetch((long long*)s.n_defined, d_nd, (size_t)n_stats, st));
    HIP_TRY(fetch((long long*)s.n_greater, d_ng, (size_t)n_stats, st));
    HIP_TRY(fetch((long long*)s.n_equal, d_ne, (size_t)n_stats, st));
    HIP_TRY(fetch(s.mean_obs, d_mo, (size_t)n_stats, st));
    HIP_TRY(fetch(s.mean_rep, d_mr, (size_t)n_stats, st));
    HIP_TRY(fetch(s.var_rep, d_vr, (size_t)n_stats, st));
    HIP_TRY(fetch(s.t_obs ? tobs_h.data() : nullptr, d_tobs, (size_t)U * n_stats, st));
    HIP_TRY(fetch(s.t_rep, d_trep, (size_t)M * n_stats, st));
    HIP_TRY(fetch(s.z, d_z, (size_t)M * N, st));
    HIP_TRY(fetch(s.y_rep, d_yrep, (size_t)M * N, st));
    if (int rc = wait_stream(h)) return rc;
    for (long long i = 0; s.t_obs && i < M; ++i)
        std::copy_n(tobs_h.begin() + (size_t)occ_u[(size_t)i] * n_stats, n_stats, s.t_obs + (size_t)i * n_stats);
    return 0;
}

// ---- power-scaling sensitivity (ptnn_dev_powerscale.hpp) ----
static_assert(PTNN_POWERSCALE_MAX_DISTINCT == PS_MAX_DISTINCT, "ptnn.h powerscale limits");

// one block of nq quantities whose sort words are in `keys`: order them, then the distances and moments of the four perturbations
static int powerscale_block(ptnn_handle* h, unsigned long long* keys, int nq, int npow, PsDist da, int q0) {
    if (int rc = sort_segments(h, keys, nq, npow)) return rc;
    da.keys = keys; da.q0 = q0;
    HIP_TRY(launch(powerscale_distance_kernel, dim3((unsigned)nq, 4), dim3(PS_THREADS), 0, h->stream, da));
    return 0;
}

int ptnn_powerscale(ptnn_handle* h, const ptnn_powerscale_spec* spec) {
    // argument checks first: none of them needs the handle or a device
    if (int rc = check_spec(spec, "ptnn_powerscale_spec")) return rc;
    const ptnn_powerscale_spec& s = *spec;
    RowsByVectors f(s, x_rows(s), s.w != nullptr);
    constexpr int all_groups = PTNN_POWERSCALE_WEIGHTS | PTNN_POWERSCALE_ETA | PTNN_POWERSCALE_PREDICTIONS | PTNN_POWERSCALE_LOGLIK;
    const bool g_w = s.groups & PTNN_POWERSCALE_WEIGHTS, g_eta = s.groups & PTNN_POWERSCALE_ETA,
               g_pred = s.groups & PTNN_POWERSCALE_PREDICTIONS, g_ll = s.groups & PTNN_POWERSCALE_LOGLIK;
    if (!(s.delta > 0.0) || !std::isfinite(s.delta)) return fail(-1, "delta = %g must be a finite number > 0", s.delta);
    if (int rc = check_r_eff(s.r_eff)) return rc;
    if (s.groups == 0 || (s.groups & ~all_groups))
        return fail(-1, "groups = 0x%x: choose among PTNN_POWERSCALE_WEIGHTS, _ETA, _PREDICTIONS and _LOGLIK", (unsigned)s.groups);
    if (int rc = f.check_source()) return rc;
    if (g_pred) {
        if (s.n_rows < 1) return fail(-1, "n_rows = %d must be >= 1", s.n_rows);
        if (int rc = check_rows(f.rows)) return rc;
    }
    if (int rc = f.count_host()) return rc;
    if (int rc = check_handle(h, "ptnn_powerscale")) return rc;
    const int I = h->cfg.n_in, H = h->cfg.n_hidden, O = h->cfg.n_out, P = h->P, Ntr = h->Ntr;
    const bool reg = h->cfg.task == PTNN_TASK_REG;
    if (g_eta && !reg) return fail(-1, "PTNN_POWERSCALE_ETA: a classification has no eta");
    if (int rc = f.fit(h, g_pred)) return rc;
    if (int rc = f.select(h, nullptr, "importance weights need at least 2")) return rc;
    const long long M = f.M;
    long long Mt = 0;
    if (int rc = psis_tail(M, s.r_eff, &Mt)) return rc;
    const long long n_pred = g_pred ? (long long)s.n_rows * O : 0;
    const long long Qll = (g_w ? P : 0) + (g_eta ? 1 : 0) + n_pred + (g_ll ? 1 : 0);
    if (Qll > 0x7fffffffLL) return fail(-1, "%lld quantities: at most 2^31 - 1 per call", Qll);
    const int Q = (int)Qll;
    if (s.n_samples) *s.n_samples = M;
    if (s.n_quantities) *s.n_quantities = Q;

    // stage a: items -> distinct (w, eta) samples (a classification's: distinct w); the rows follow with the predictions
    f.eta = reg;
    if (int rc = f.stage(h, 0, s.n_distinct)) return rc;
    hipStream_t st = h->stream;
    DeviceScratch& mem = f.mem;
    const Distinct& d = f.d;
    const int U = f.U;
    if (U > PS_MAX_DISTINCT)
        return fail(-1, "%d distinct samples: power-scaling orders every quantity over all of them, at most %d; thin= lowers the "
                        "number of distinct samples", U, PS_MAX_DISTINCT);
    const size_t budget = scratch_budget("PTNN_POWERSCALE_SCRATCH_BYTES");
    const ForwardPlan& fwd = f.fwd;
    if (int rc = f.fwd.init(h, "power-scaling sensitivity")) return rc;

    // 1. the components: l_u over the training rows in blocks of rows, pi_u from w and eta
    double* d_logp = nullptr;
    HIP_TRY(mem.alloc(&d_logp, (size_t)2 * U));
    HIP_TRY(hipMemsetAsync(d_logp, 0, (size_t)U * sizeof(double), st));
    {
        DeviceScratch tmp;
        const long long rows_blk = row_block(budget, (size_t)U * (sizeof(float) * O + sizeof(double)), Ntr);
        float* d_fx = nullptr;
        double* d_llb = nullptr;
        HIP_TRY(tmp.alloc(&d_fx, (size_t)rows_blk * O * U));
        HIP_TRY(tmp.alloc(&d_llb, (size_t)rows_blk * U));
        ElpdRed ra{};
        ra.mode = reg ? ELPD_REG : ELPD_CLS; ra.eta = d.run_eta; ra.cnt = d.run_cnt; ra.U = U; ra.O = O;
        if (int rc = each_block(Ntr, rows_blk, [&](long long r0, int nr) -> int {
            if (int rc = loglik_rows(h, fwd, d, h->d_data, h->IPY, r0, nr, d_fx, d_llb, ra)) return rc;
            HIP_TRY(launch(powerscale_loglik_kernel, dim3((unsigned)((U + PS_THREADS - 1) / PS_THREADS)), dim3(PS_THREADS), 0, st, d_llb, nr, U, d_logp));
            return 0;
        })) return rc;
        if (int rc = wait_stream(h)) return rc;          // `tmp` is released here
    }
    const double sig2 = (double)h->cfg.sigma_squared;
    const double cnt = reg ? (double)(I * H + H + 2) : (double)(I * H + H + O + H * O);
    PsPrior pa{d.base, d.run_off, d.run_eta, U, P, reg ? 1 : 0, -1.0 * (cnt / 2.0) * std::log(sig2), 1.0 / (2.0 * sig2),
               (double)h->cfg.nu_1, (double)h->cfg.nu_2, d_logp + U};
    HIP_TRY(launch(powerscale_prior_kernel, dim3((unsigned)((U + PS_THREADS / WAVE - 1) / (PS_THREADS / WAVE))), dim3(PS_THREADS), 0, st, pa));
    std::vector<double> logp_h((size_t)2 * U);
    std::vector<int> cnt_h((size_t)U);
    HIP_TRY(hipMemcpyAsync(logp_h.data(), d_logp, logp_h.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(cnt_h.data(), d.run_cnt, cnt_h.size() * sizeof(int), hipMemcpyDeviceToHost, st));
    if (int rc = wait_stream(h)) return rc;
    for (int c = 0; c < 2; ++c)
        for (int u = 0; u < U; ++u)
            if (cnt_h[(size_t)u] > 0 && !std::isfinite(logp_h[(size_t)c * U + u]))
                return fail(-1, "the %s component of distinct sample %d is %g: power-scaling needs finite log-%s values for every selected "
                                "sample", c ? "prior" : "likelihood", u, logp_h[(size_t)c * U + u], c ? "prior" : "likelihood");
    if (s.logp) std::copy(logp_h.begin(), logp_h.end(), s.logp);

    // 2. the smoothed, normalised weights of the four perturbations
    double *d_wt = nullptr, *d_tlw = nullptr, *d_khat = nullptr;
    int *d_tu = nullptr, *d_live = nullptr;
    long long* d_tail = nullptr;
    HIP_TRY(mem.alloc(&d_wt, (size_t)4 * U));
    HIP_TRY(mem.alloc(&d_tlw, (size_t)4 * ELPD_TAIL_CAP));
    HIP_TRY(mem.alloc(&d_tu, (size_t)4 * ELPD_TAIL_CAP));
    HIP_TRY(mem.alloc(&d_khat, 4));
    HIP_TRY(mem.alloc(&d_tail, 4));
    HIP_TRY(mem.alloc(&d_live, 1));
    const double a_plus = 1.0 + s.delta, a_minus = 1.0 / (1.0 + s.delta);
    if (int rc = raise_lds_limit(reinterpret_cast<const void*>(powerscale_smooth_kernel), LFO_LDS_BYTES)) return rc;
    PsSmooth sa{d_logp, d.run_cnt, U, (int)Mt, M, {a_minus - 1.0, a_plus - 1.0}, d_wt, d_tlw, d_tu, d_khat, d_tail, d_live};
    HIP_TRY(launch(powerscale_smooth_kernel, dim3(4), dim3(ELPD_THREADS), LFO_LDS_BYTES, st, sa));

    // 3, 4. the quantities in blocks of whole quantities
    int npow = 2;
    while (npow < U) npow <<= 1;
    const size_t per_q = sizeof(unsigned long long) * (size_t)npow + sizeof(float) * (size_t)U;
    const int Qb = (int)std::max<size_t>(1, std::min<size_t>({budget / per_q, (size_t)65535, (size_t)Q}));
    const int rows_q = g_pred ? std::max(1, std::min(Qb / O, s.n_rows)) : 0;      // rows of predictions per block
    const int cap_q = std::max(Qb, rows_q * O);
    unsigned long long* d_keys = nullptr;
    float* d_fx = nullptr;
    double *d_dist = nullptr, *d_mean = nullptr, *d_sd = nullptr, *d_bmean = nullptr, *d_bsd = nullptr;
    HIP_TRY(mem.alloc(&d_keys, (size_t)cap_q * npow));
    if (g_pred) HIP_TRY(mem.alloc(&d_fx, (size_t)rows_q * O * U));
    HIP_TRY(mem.alloc(&d_dist, (size_t)4 * Q));
    HIP_TRY(mem.alloc(&d_mean, (size_t)4 * Q));
    HIP_TRY(mem.alloc(&d_sd, (size_t)4 * Q));
    HIP_TRY(mem.alloc(&d_bmean, (size_t)Q));
    HIP_TRY(mem.alloc(&d_bsd, (size_t)Q));
    PsDist da{};
    da.cnt = d.run_cnt; da.wt = d_wt; da.n_live = d_live; da.U = U; da.npow = npow; da.Q = Q; da.M = (double)M;
    da.dist = d_dist; da.mean = d_mean; da.sd = d_sd; da.base_mean = d_bmean; da.base_sd = d_bsd;
    const unsigned key_blocks = (unsigned)((npow + PS_THREADS - 1) / PS_THREADS);
    auto plain = [&](const float* v32, const double* v64, int nq, int q0) -> int {      // quantities that lie [quantity][vector]
        PsKeys ka{v32, v64, d.run_cnt, U, npow, d_keys};
        HIP_TRY(launch(powerscale_keys_kernel, dim3(key_blocks, (unsigned)nq), dim3(PS_THREADS), 0, st, ka));
        return powerscale_block(h, d_keys, nq, npow, da, q0);
    };
    int q_at = 0;
    for (int p0 = 0; g_w && p0 < P; p0 += Qb) {
        const int nq = std::min(Qb, P - p0);
        PsGather ga{d.base, d.run_off, d.run_cnt, U, npow, p0, nq, d_keys};
        HIP_TRY(launch(powerscale_gather_kernel, dim3((unsigned)(npow + PS_GATHER_TILE - 1) / PS_GATHER_TILE,
                                                      (unsigned)(nq + PS_GATHER_TILE - 1) / PS_GATHER_TILE), dim3(PS_THREADS), 0, st, ga));
        if (int rc = powerscale_block(h, d_keys, nq, npow, da, q_at + p0)) return rc;
    }
    q_at += g_w ? P : 0;
    if (g_eta) {
        if (int rc = plain(d.run_eta, nullptr, 1, q_at)) return rc;
        q_at += 1;
    }
    if (g_pred) {
        if (int rc = upload_rows(h, mem, f.rows, I, &f.d_x, &f.xs)) return rc;
        f.rows_blk = rows_q; f.d_fx = d_fx;              // the predictions' blocks share the budget of the quantities
        if (int rc = f.each_rows(h, s.n_rows, [&](long long r0, int nr) { return plain(d_fx, nullptr, nr * O, q_at + (int)r0 * O); })) return rc;
        q_at += (int)n_pred;
    }
    if (g_ll)
        if (int rc = plain(nullptr, d_logp, 1, q_at)) return rc;

    std::vector<double> dist_h(s.sens || s.dist ? (size_t)4 * Q : 0);
    long long tail_h[4];
    HIP_TRY(fetch(dist_h.empty() ? nullptr : dist_h.data(), d_dist, (size_t)4 * Q, st));
    HIP_TRY(fetch(s.mean, d_mean, (size_t)4 * Q, st));
    HIP_TRY(fetch(s.sd, d_sd, (size_t)4 * Q, st));
    HIP_TRY(fetch(s.base_mean, d_bmean, (size_t)Q, st));
    HIP_TRY(fetch(s.base_sd, d_bsd, (size_t)Q, st));
    HIP_TRY(fetch(s.khat, d_khat, 4, st));
    HIP_TRY(fetch(s.tail_len ? tail_h : nullptr, d_tail, 4, st));
    if (int rc = wait_stream(h)) return rc;
    if (s.tail_len) std::copy_n(tail_h, 4, s.tail_len);
    if (s.dist) std::copy(dist_h.begin(), dist_h.end(), s.dist);
    const double scale = 2.0 * std::log2(a_plus);
    for (int c = 0; s.sens && c < 2; ++c)
        for (int q = 0; q < Q; ++q) s.sens[(size_t)c * Q + q] = (dist_h[(size_t)(2 * c) * Q + q] + dist_h[(size_t)(2 * c + 1) * Q + q]) / scale;
    return 0;
}

// ---- prior predictive checks (ptnn_dev_prior.hpp) ----
static_assert(PTNN_PRIOR_MAX_SCALES == PRIOR_MAX_SCALES, "ptnn.h prior limits");

int ptnn_prior_predictive(ptnn_handle* h, const ptnn_prior_spec* spec) {
    // argument checks first: none of them needs the handle or a device
    if (int rc = check_spec(spec, "ptnn_prior_spec")) return rc;
    const ptnn_prior_spec& s = *spec;
    const RowSource rows{s.x_source, s.x, s.n_rows, "x_source", "PTNN_PREDICT_X", "x", "n_rows"};
    RankOutputs rk{s.n_ranks, s.ranks, s.order_stats};
    if (s.n_draws < 1) return fail(-1, "n_draws = %lld must be >= 1", (long long)s.n_draws);
    if (s.draw0 < 0 || s.draw0 > (1LL << 32) || s.n_draws > (1LL << 32) - s.draw0)
        return fail(-1, "draws [%lld, %lld + %lld) outside the Philox counter's [0, 2^32)", (long long)s.draw0, (long long)s.draw0,
                    (long long)s.n_draws);
    if (s.n_scales < 0 || s.n_scales > PRIOR_MAX_SCALES) return fail(-1, "n_scales = %d outside [0, %d]", s.n_scales, PRIOR_MAX_SCALES);
    if (s.n_scales > 0 && !s.sigma_squared) return fail(-1, "n_scales = %d but sigma_squared is NULL", s.n_scales);
    for (int k = 0; k < s.n_scales; ++k)
        if (!(s.sigma_squared[k] > 0.0) || !std::isfinite(s.sigma_squared[k]))
            return fail(-1, "sigma_squared[%d] = %g must be a finite number > 0", k, s.sigma_squared[k]);
    if (!(s.eps > 0.0 && s.eps < 0.5)) return fail(-1, "eps = %g must lie in (0, 0.5)", s.eps);
    if (int rc = check_rows(rows)) return rc;
    if (s.n_rows < 1) return fail(-1, "n_rows = %d must be >= 1", s.n_rows);
    if (int rc = rk.check()) return rc;
    if (s.stat_order_stats && s.n_ranks == 0) return fail(-1, "stat_order_stats requested without ranks");
    if (int rc = check_handle(h, "ptnn_prior_predictive")) return rc;
    const int I = h->cfg.n_in, O = h->cfg.n_out, P = h->P, N = s.n_rows;
    const bool reg = h->cfg.task == PTNN_TASK_REG;
    if (reg && O != 1) return fail(-1, "a regression's prior predictive check needs n_out == 1; this handle has n_out = %d", O);
    if (s.vote && reg) return fail(-1, "vote: a regression has no classes");
    if (int rc = fit_rows(h, rows)) return rc;
    const bool has_y = s.x_source != PTNN_PREDICT_X_HOST || s.has_target != 0;
    if (s.x_source == PTNN_PREDICT_X_HOST && has_y && !reg)
        for (int n = 0; n < N; ++n) {
            const float yv = s.x[(size_t)n * (I + 1) + I];
            if (!(yv >= 0.0f) || yv >= (float)O || yv != std::floor(yv))
                return fail(-1, "class label %g in row %d is not an integer in [0, %d)", (double)yv, n, O);
        }
    const long long ncols_all = (long long)N * O, ND = s.n_draws;
    if (ncols_all > 0x7fffffffLL) return fail(-1, "%d rows x %d outputs = %lld columns: at most 2^31 - 1 per call", N, O, ncols_all);
    const int ncols = (int)ncols_all;
    const size_t budget = scratch_budget("PTNN_PRIOR_SCRATCH_BYTES");
    const long long fits = (long long)(budget / ((size_t)ncols * sizeof(float)));
    if (ND > fits)
        return fail(-1, "n_draws = %lld: the outputs of one scale, 4 x %d rows x %d outputs x n_draws bytes, exceed the scratch budget of "
                        "%zu bytes ($PTNN_PRIOR_SCRATCH_BYTES); the largest n_draws that fits is %lld -- a prior predictive check needs "
                        "thousands of draws, not millions", ND, N, O, budget, fits);
    if (ND > 0x7fffffffLL) return fail(-1, "%lld draws: at most 2^31 - 1 per call", ND);
    if (int rc = rk.check_values(ND)) return rc;
    const int n_stats = reg ? PRIOR_REG_STATS : PRIOR_CLS_FIXED + O;
    const int S = std::max(1, s.n_scales);
    if (s.n_stats) *s.n_stats = n_stats;

    if (int rc = start_device(h)) return rc;
    hipStream_t st = h->stream;
    DeviceScratch mem;
    const float* d_x = nullptr;
    int xs = 0;
    if (int rc = upload_rows(h, mem, rows, I + (has_y ? 1 : 0), &d_x, &xs)) return rc;
    const float* d_y = has_y ? d_x + I : nullptr;
    // blocks of draws: what the budget leaves beside the scale's output matrix, at least one draw; rows in blocks of predict_fwd's grid
    const long long rows_blk = std::min<long long>(N, 65535LL * WAVE);
    const size_t per_draw = (size_t)P * sizeof(float) + sizeof(long long) + (size_t)rows_blk * O * sizeof(float);
    const long long nb = std::max(1LL, std::min<long long>((long long)((budget - (size_t)ncols * ND * sizeof(float)) / per_draw), ND));
    if (s.n_blocks) *s.n_blocks = (ND + nb - 1) / nb;
    float *d_fx = nullptr, *d_fxb = nullptr, *d_pw = nullptr, *d_t32 = nullptr, *d_tos = nullptr;
    long long *d_poff = nullptr, *d_sat = nullptr, *d_cnt = nullptr, *d_tranks = nullptr;
    int* d_ones = nullptr;
    double *d_mean = nullptr, *d_t = nullptr, *d_tobs = nullptr, *d_tm = nullptr, *d_tmean = nullptr;
    HIP_TRY(mem.alloc(&d_fx, (size_t)ncols * ND));
    HIP_TRY(mem.alloc(&d_fxb, (size_t)rows_blk * O * nb));
    HIP_TRY(mem.alloc(&d_pw, (size_t)nb * P));
    HIP_TRY(mem.alloc(&d_poff, (size_t)nb));
    HIP_TRY(mem.alloc(&d_ones, (size_t)ND));
    HIP_TRY(hipMemsetD32Async(d_ones, 1, (size_t)ND, st));
    HIP_TRY(mem.alloc(&d_mean, (size_t)ncols));
    if (int rc = rk.to_device(mem, (size_t)ncols, st)) return rc;
    PooledVotes votes;
    if (!reg) HIP_TRY(votes.alloc(mem, (size_t)ncols));
    HIP_TRY(mem.alloc(&d_sat, (size_t)ncols));
    HIP_TRY(mem.alloc(&d_t, (size_t)n_stats * ND));
    HIP_TRY(mem.alloc(&d_t32, (size_t)n_stats * ND));
    HIP_TRY(mem.alloc(&d_tobs, (size_t)n_stats));
    HIP_TRY(mem.alloc(&d_tm, (size_t)2 * n_stats));            // stat_mean, stat_sd
    HIP_TRY(mem.alloc(&d_tmean, (size_t)n_stats));             // predict_reduce_kernel's mean of the fp32 copy: not used
    HIP_TRY(mem.alloc(&d_cnt, (size_t)3 * n_stats));           // n_greater, n_equal, n_defined
    if (s.n_ranks) HIP_TRY(mem.alloc(&d_tos, (size_t)s.n_ranks * n_stats));
    d_tranks = rk.d_ranks;
    ForwardPlan fwd;
    if (int rc = fwd.init(h, "prior predictive check")) return rc;
    uint32_t slo = 0, shi = 0;
    split_seed(s.seed, &slo, &shi);
    const int nq = (P + 3) / 4;
    HIP_TRY(launch(reg ? prior_target_kernel<true> : prior_target_kernel<false>, dim3(1), dim3(WAVE), 0, st, d_y, xs, N, O, d_tobs));
    HIP_TRY(fetch(s.t_obs, d_tobs, (size_t)n_stats, st));
    std::vector<int> identity(s.samples || s.t_draw ? (size_t)ND : 0);
    for (size_t i = 0; i < identity.size(); ++i) identity[i] = (int)i;

    for (int k = 0; k < S; ++k) {
        const float sigma = (float)std::sqrt(s.n_scales ? s.sigma_squared[k] : (double)h->cfg.sigma_squared);
        // stages a, b: the scale's outputs fx [ncols][ND], a block of draws at a time
        for (long long d0 = 0; d0 < ND; d0 += nb) {
            const int b = (int)std::min<long long>(nb, ND - d0);
            HIP_TRY(launch(evid_prior_kernel, dim3((unsigned)(((long long)b * nq + EVID_THREADS - 1) / EVID_THREADS)), dim3(EVID_THREADS), 0, st,
                           s.draw0 + d0, b, P, sigma, slo, shi, d_pw, d_poff));
            if (s.weights)
                HIP_TRY(hipMemcpyAsync(s.weights + ((size_t)k * ND + d0) * P, d_pw, (size_t)b * P * sizeof(float), hipMemcpyDeviceToHost, st));
            if (int rc = each_block(N, rows_blk, [&](long long r0, int nr) -> int {
                if (int rc = fwd.run(h, d_pw, d_poff, d_x, xs, (int)r0, nr, b, d_fxb)) return rc;
                HIP_TRY(hipMemcpy2DAsync(d_fx + (size_t)r0 * O * ND + d0, (size_t)ND * sizeof(float), d_fxb, (size_t)b * sizeof(float),
                                         (size_t)b * sizeof(float), (size_t)nr * O, hipMemcpyDeviceToDevice, st));
                return 0;
            })) return rc;
        }
        // stage c: every column over the draws
        PredictRed ra{d_fx, d_ones, (int)ND, O, 0, ncols, ND, s.n_ranks, rk.d_ranks, d_mean, rk.d_stats, votes.d};
        HIP_TRY(launch(predict_reduce_kernel, dim3((unsigned)ncols), dim3(PRED_THREADS), 0, st, ra));
        HIP_TRY(launch(prior_saturation_kernel, dim3((unsigned)ncols), dim3(PRIOR_THREADS), 0, st, d_fx, ND, s.eps, d_sat));
        // stage d: every draw over the rows; the order statistics of the fp32 copy
        PriorFn fa{d_fx, ND, N, O, d_y, xs, s.eps, d_t, d_t32};
        HIP_TRY(launch(reg ? prior_function_kernel<true> : prior_function_kernel<false>, dim3((unsigned)((ND + PRIOR_THREADS - 1) / PRIOR_THREADS)),
                       dim3(PRIOR_THREADS), 0, st, fa));
        if (s.n_ranks) {
            PredictRed ta{d_t32, d_ones, (int)ND, 1, 0, n_stats, ND, s.n_ranks, d_tranks, d_tmean, d_tos, nullptr};
            HIP_TRY(launch(predict_reduce_kernel, dim3((unsigned)n_stats), dim3(PRED_THREADS), 0, st, ta));
        }
        // stage e: every statistic over the draws
        PriorStat sa{d_t, ND, d_tobs, d_tm, d_tm + n_stats, d_cnt, d_cnt + n_stats, d_cnt + 2 * n_stats};
        HIP_TRY(launch(prior_stat_kernel, dim3((unsigned)n_stats), dim3(PRIOR_THREADS), 0, st, sa));
        const size_t kc = (size_t)k * ncols, kt = (size_t)k * n_stats;
        HIP_TRY(fetch(s.mean ? s.mean + kc : nullptr, d_mean, (size_t)ncols, st));
        HIP_TRY(fetch(s.order_stats ? s.order_stats + kc * s.n_ranks : nullptr, rk.d_stats, (size_t)s.n_ranks * ncols, st));
        HIP_TRY(votes.fetch(s.vote != nullptr, (size_t)ncols, st));
        HIP_TRY(fetch(s.sat_count ? (long long*)s.sat_count + kc : nullptr, d_sat, (size_t)ncols, st));
        HIP_TRY(fetch(s.stat_mean ? s.stat_mean + kt : nullptr, d_tm, (size_t)n_stats, st));
        HIP_TRY(fetch(s.stat_sd ? s.stat_sd + kt : nullptr, d_tm + n_stats, (size_t)n_stats, st));
        HIP_TRY(fetch(s.stat_order_stats ? s.stat_order_stats + kt * s.n_ranks : nullptr, d_tos, (size_t)s.n_ranks * n_stats, st));
        HIP_TRY(fetch(s.n_greater ? (long long*)s.n_greater + kt : nullptr, d_cnt, (size_t)n_stats, st));
        HIP_TRY(fetch(s.n_equal ? (long long*)s.n_equal + kt : nullptr, d_cnt + n_stats, (size_t)n_stats, st));
        HIP_TRY(fetch(s.n_defined ? (long long*)s.n_defined + kt : nullptr, d_cnt + 2 * n_stats, (size_t)n_stats, st));
        if (s.t_draw)
            if (int rc = scatter_samples(h, d_t, n_stats, (int)ND, identity, nullptr, s.t_draw + kt * ND, (size_t)n_stats, 0)) return rc;
        if (s.samples)
            if (int rc = scatter_samples(h, d_fx, ncols, (int)ND, identity, nullptr, s.samples + kc * ND, (size_t)ncols, 0)) return rc;
        if (int rc = wait_stream(h)) return rc;
        if (s.vote) votes.shares(s.vote + kc, ND);
    }
    return 0;
}

// ---- classification report (ptnn_dev_report.hpp) ----
static_assert(PTNN_REPORT_MAX_AUC_ROWS == REPORT_MAX_AUC_ROWS, "ptnn.h report limits");

int ptnn_class_report(ptnn_handle* h, const ptnn_class_report_spec* spec) {
    // argument checks first: none of them needs the handle or a device
    if (int rc = check_spec(spec, "ptnn_class_report_spec")) return rc;
    const ptnn_class_report_spec& s = *spec;
    RowsByVectors f(s, RankOutputs{s.n_ranks, s.ranks, s.metric_order_stats});
    if (int rc = f.check(true)) return rc;
    if (s.auc && s.n_rows > REPORT_MAX_AUC_ROWS)
        return fail(-1, "auc: %d rows, at most %d (the scores of one sample and class are ranked in LDS); auc = 0 (auc=False) has no cap",
                    s.n_rows, REPORT_MAX_AUC_ROWS);
    if (int rc = check_handle(h, "ptnn_class_report")) return rc;
    const int I = h->cfg.n_in, K = h->cfg.n_out, KK = K * K, N = s.n_rows;
    if (h->cfg.task != PTNN_TASK_CLS) return fail(-1, "ptnn_class_report: a regression has no classes");
    if (int rc = fit_rows(h, f.rows)) return rc;
    if (s.x_source == PTNN_PREDICT_X_HOST)
        if (int rc = check_labels(s.x, N, I, K)) return rc;
    if (int rc = f.select(h, s.n_samples)) return rc;

    if (int rc = f.stage(h, I + 1, s.n_distinct)) return rc;
    hipStream_t st = h->stream;
    DeviceScratch& mem = f.mem;
    const Distinct& d = f.d;
    RankOutputs& rk = f.rk;
    const float* d_x = f.d_x;
    const long long M = f.M;
    const int xs = f.xs, U = f.U, ncols = N * K, Q = s.auc ? 4 + 4 * K : 3 + 3 * K;
    // the class of every row as an integer: the kernels' index, and on the host p_correct's
    int* d_label = nullptr;
    HIP_TRY(mem.alloc(&d_label, (size_t)N));
    HIP_TRY(launch(report_labels_kernel, dim3((unsigned)((N + REPORT_THREADS - 1) / REPORT_THREADS)), dim3(REPORT_THREADS), 0, st, d_x + I, xs, N, K,
                   d_label));
    std::vector<int> label_h((size_t)N);
    HIP_TRY(hipMemcpyAsync(label_h.data(), d_label, (size_t)N * sizeof(int), hipMemcpyDeviceToHost, st));
    // per column of the pooled classifier, per sample, per metric
    double *d_mean = nullptr, *d_mmean = nullptr;
    long long *d_auc2 = nullptr, *d_csum = nullptr;
    PooledVotes votes;
    int* d_conf = nullptr;
    float* d_img = nullptr;
    HIP_TRY(mem.alloc(&d_mean, (size_t)ncols));
    HIP_TRY(votes.alloc(mem, (size_t)ncols));
    HIP_TRY(mem.alloc(&d_conf, (size_t)KK * U));
    HIP_TRY(hipMemsetAsync(d_conf, 0, (size_t)KK * U * sizeof(int), st));
    if (s.auc) HIP_TRY(mem.alloc(&d_auc2, (size_t)K * U));
    HIP_TRY(mem.alloc(&d_img, (size_t)Q * U));
    HIP_TRY(mem.alloc(&d_mmean, (size_t)Q));
    HIP_TRY(mem.alloc(&d_csum, (size_t)KK));
    if (int rc = rk.to_device(mem, (size_t)Q, st)) return rc;
    // The forward image: all rows of all samples where that fits the budget; else the pooled classifier from ptnn_predict's blocks
    // of rows, then everything per sample from blocks of samples (a sample's AUC needs all its rows at once)
    const size_t budget = scratch_budget("PTNN_REPORT_SCRATCH_BYTES");
    const size_t row_bytes = (size_t)U * sizeof(float) * K, sample_bytes = (size_t)N * sizeof(float) * K;
    const bool one_pass = row_bytes * N <= budget;
    const long long rows_blk = one_pass ? N : row_block(budget, row_bytes, N);
    const long long u_blk = one_pass ? U : std::max<long long>(1, std::min<long long>(U, (long long)(budget / sample_bytes)));
    float* d_fx = nullptr;
    HIP_TRY(mem.alloc(&d_fx, std::max((size_t)rows_blk * K * U, (size_t)u_blk * N * K)));
    ForwardPlan fwd;
    if (int rc = fwd.init(h, "classification report")) return rc;
    int TU = WAVE;
    while (TU > 1 && (size_t)KK * TU * sizeof(int) > (size_t)REPORT_CONF_LDS) TU >>= 1;
    const size_t conf_lds = (size_t)KK * TU * sizeof(int);
    if (conf_lds > LDS_CEILING) return fail(-3, "classification report: the counts of %d classes do not fit in LDS", K);
    if (int rc = raise_lds_limit(reinterpret_cast<const void*>(report_confusion_kernel), conf_lds)) return rc;
    const int rows_per_group = std::max(WAVE, (N + 7) / 8);
    int npow = 1;
    while (npow < N) npow <<= 1;
    const bool small = npow <= REPORT_SORT_SMALL;
    const size_t auc_lds = ((size_t)npow + (small ? REPORT_THREADS : REPORT_SORT_THREADS)) * sizeof(unsigned long long);
    if (s.auc && !small)
        if (int rc = raise_lds_limit(reinterpret_cast<const void*>(report_auc_kernel<REPORT_SORT_THREADS>), auc_lds)) return rc;
    // the integers of samples [u0, u0 + nb), whose outputs on all rows are d_fx [ncols][nb]
    const auto count_block = [&](long long u0, int nb) -> int {
        ReportConf ca{d_fx, d_label, N, K, nb, TU, rows_per_group, U, (int)u0, d_conf};
        HIP_TRY(launch(report_confusion_kernel, dim3((unsigned)((nb + TU - 1) / TU), (unsigned)((N + rows_per_group - 1) / rows_per_group)),
                       dim3(REPORT_THREADS), conf_lds, st, ca));
        if (!s.auc) return 0;
        ReportAuc aa{d_fx, d_label, N, K, nb, npow, U, (int)u0, d_auc2};
        if (small) HIP_TRY(launch(report_auc_kernel<REPORT_THREADS>, dim3((unsigned)nb, (unsigned)K), dim3(REPORT_THREADS), auc_lds, st, aa));
        else HIP_TRY(launch(report_auc_kernel<REPORT_SORT_THREADS>, dim3((unsigned)nb, (unsigned)K), dim3(REPORT_SORT_THREADS), auc_lds, st, aa));
        return 0;
    };
    if (int rc = each_block(N, rows_blk, [&](long long r0, int nr) -> int {
        if (int rc = fwd.run(h, d.base, d.run_off, d_x, xs, (int)r0, nr, U, d_fx)) return rc;
        PredictRed ra{d_fx, d.run_cnt, U, K, (int)r0 * K, ncols, M, 0, nullptr, d_mean, nullptr, votes.d};
        HIP_TRY(launch(predict_reduce_kernel, dim3((unsigned)(nr * K)), dim3(PRED_THREADS), 0, st, ra));
        return one_pass ? count_block(0, U) : 0;
    })) return rc;
    if (!one_pass)
        if (int rc = each_block(U, u_blk, [&](long long u0, int nb) -> int {
            if (int rc = fwd.run(h, d.base, d.run_off + u0, d_x, xs, 0, N, nb, d_fx)) return rc;
            return count_block(u0, nb);
        })) return rc;
    // the metric columns of every sample, reduced over the samples as ptnn_predict reduces a column of outputs
    ReportMetrics ma{d_conf, d_auc2, U, K, N, d_img};
    HIP_TRY(launch(report_metrics_kernel, dim3((unsigned)((U + REPORT_THREADS - 1) / REPORT_THREADS)), dim3(REPORT_THREADS), 0, st, ma));
    PredictRed qa{d_img, d.run_cnt, U, 1, 0, Q, M, s.n_ranks, rk.d_ranks, d_mmean, rk.d_stats, nullptr};
    HIP_TRY(launch(predict_reduce_kernel, dim3((unsigned)Q), dim3(PRED_THREADS), 0, st, qa));
    HIP_TRY(launch(report_confusion_sum_kernel, dim3((unsigned)KK), dim3(REPORT_THREADS), 0, st, d_conf, d.run_cnt, U, d_csum));
    HIP_TRY(fetch(s.p_mean, d_mean, (size_t)ncols, st));
    HIP_TRY(votes.fetch(s.vote || s.p_correct, (size_t)ncols, st));
    HIP_TRY(fetch(s.metric_mean, d_mmean, (size_t)Q, st));
    HIP_TRY(fetch(s.metric_order_stats, rk.d_stats, (size_t)s.n_ranks * Q, st));
    HIP_TRY(fetch((long long*)s.confusion_sum, d_csum, (size_t)KK, st));
    if (s.sample_metrics || s.sample_confusion) {
        if (int rc = f.items(h, true)) return rc;
        if (int rc = wait_stream(h)) return rc;
        if (s.sample_metrics)
            if (int rc = scatter_samples(h, d_img, Q, U, f.item_run, f.src.weights(), s.sample_metrics, (size_t)Q, 0)) return rc;
        if (s.sample_confusion)
            if (int rc = scatter_samples(h, d_conf, KK, U, f.item_run, f.src.weights(), s.sample_confusion, (size_t)KK, 0)) return rc;
    }
    if (int rc = wait_stream(h)) return rc;
    for (int n = 0; n < N; ++n)
        if (label_h[(size_t)n] < 0) return fail(-2, "row %d of the handle's data has no class in [0, %d) (internal error)", n, K);
    votes.shares(s.vote, M);
    for (int n = 0; s.p_correct && n < N; ++n) s.p_correct[n] = votes.share((size_t)n * K + label_h[(size_t)n], M);
    return 0;
}

// ---- predictive uncertainty (ptnn_dev_uncertainty.hpp) ----
int ptnn_uncertainty(ptnn_handle* h, const ptnn_uncertainty_spec* spec) {
    // argument checks first: none of them needs the handle or a device
    if (int rc = check_spec(spec, "ptnn_uncertainty_spec")) return rc;
    const ptnn_uncertainty_spec& s = *spec;
    RowsByVectors f(s, x_rows(s), s.w != nullptr, RankOutputs{s.n_ranks, s.ranks, s.entropy_order_stats});
    RankOutputs& rk = f.rk;
    if (int rc = f.check_source()) return rc;
    if (int rc = check_rows(f.rows)) return rc;
    if (s.n_rows < 1) return fail(-1, "n_rows = %d must be >= 1", s.n_rows);
    if (int rc = rk.check()) return rc;
    if (int rc = f.count_host()) return rc;
    if (int rc = check_handle(h, "ptnn_uncertainty")) return rc;
    const int I = h->cfg.n_in, O = h->cfg.n_out, N = s.n_rows;
    const bool reg = h->cfg.task == PTNN_TASK_REG;
    if (reg && (s.vote || s.entropy_mean || s.entropy_order_stats || s.sample_entropy))
        return fail(-1, "vote, entropy_mean, entropy_order_stats and sample_entropy: a regression has no class probabilities");
    if (!reg && (s.epistemic_var || s.aleatoric_var))
        return fail(-1, "epistemic_var and aleatoric_var: a classification has no output variance and no eta");
    if (int rc = f.fit(h)) return rc;
    if (int rc = f.select(h, s.n_samples)) return rc;
    const long long S = f.M;

    // stage a: items -> distinct (w, eta) samples (a classification's: distinct w, as ptnn_predict's)
    f.eta = reg;
    if (int rc = f.stage(h, I, s.n_distinct)) return rc;
    hipStream_t st = h->stream;
    DeviceScratch& mem = f.mem;
    const Distinct& d = f.d;
    const int ncols = N * O, U = f.U;
    // the pooled outputs of every column as ptnn_predict's; then per row the entropies, or per column the variance
    const bool image = !reg && (s.n_ranks > 0 || s.sample_entropy);
    double *d_mean = nullptr, *d_hmean = nullptr, *d_emean = nullptr, *d_var = nullptr, *d_noise = nullptr;
    PooledVotes votes;
    HIP_TRY(mem.alloc(&d_mean, (size_t)ncols));
    if (reg) {
        HIP_TRY(mem.alloc(&d_var, (size_t)ncols));
        HIP_TRY(mem.alloc(&d_noise, 1));
        HIP_TRY(launch(unc_noise_kernel, dim3(1), dim3(UNC_THREADS), 0, st, U, d.run_eta, d.run_cnt, S, d_noise));
    } else {
        HIP_TRY(votes.alloc(mem, (size_t)ncols));
        HIP_TRY(mem.alloc(&d_emean, (size_t)N));
        if (image) HIP_TRY(mem.alloc(&d_hmean, (size_t)N));     // predict_reduce_kernel's mean of the fp32 image: not an output
        if (int rc = rk.to_device(mem, (size_t)N, st)) return rc;
    }
    // stage b + c in blocks of rows: the forward image U x (rows x O) floats, and the entropy image U x rows, under the budget
    if (int rc = f.forward(h, "PTNN_UNC_SCRATCH_BYTES", 1, (size_t)U * sizeof(float) * (O + (image ? 1 : 0)), N, "predictive uncertainty")) return rc;
    float *const d_fx = f.d_fx, *d_img = nullptr;
    if (image) HIP_TRY(mem.alloc(&d_img, (size_t)f.rows_blk * U));
    if (int rc = f.items(h, !reg && s.sample_entropy)) return rc;
    const double log_k = O > 1 ? std::log((double)O) : 0.0;
    if (int rc = f.each_rows(h, N, [&](long long r0, int nr) -> int {
        PredictRed ra{d_fx, d.run_cnt, U, O, (int)r0 * O, ncols, S, 0, nullptr, d_mean, nullptr, votes.d};
        HIP_TRY(launch(predict_reduce_kernel, dim3((unsigned)(nr * O)), dim3(PRED_THREADS), 0, st, ra));
        if (reg) {
            UncVariance va{d_fx, d.run_cnt, U, (int)r0 * O, S, d_mean, d_var};
            HIP_TRY(launch(unc_variance_kernel, dim3((unsigned)(nr * O)), dim3(UNC_THREADS), 0, st, va));
            return 0;
        }
        UncEntropy ea{d_fx, d.run_cnt, U, O, (int)r0, S, log_k, d_img, d_emean};
        HIP_TRY(launch(unc_entropy_kernel, dim3((unsigned)nr), dim3(UNC_THREADS), 0, st, ea));
        if (s.n_ranks > 0) {        // the order statistics of (float)H_u, as ptnn_predict reduces a column of outputs
            PredictRed qa{d_img, d.run_cnt, U, 1, (int)r0, N, S, s.n_ranks, rk.d_ranks, d_hmean, rk.d_stats, nullptr};
            HIP_TRY(launch(predict_reduce_kernel, dim3((unsigned)nr), dim3(PRED_THREADS), 0, st, qa));
        }
        return s.sample_entropy ? scatter_samples(h, d_img, nr, U, f.item_run, f.src.weights(), s.sample_entropy, (size_t)N, (size_t)r0) : 0;
    })) return rc;
    HIP_TRY(fetch(s.mean, d_mean, (size_t)ncols, st));
    HIP_TRY(votes.fetch(s.vote != nullptr, (size_t)ncols, st));
    HIP_TRY(fetch(s.entropy_mean, d_emean, (size_t)N, st));
    HIP_TRY(fetch(s.entropy_order_stats, rk.d_stats, (size_t)s.n_ranks * N, st));
    HIP_TRY(fetch(s.epistemic_var, d_var, (size_t)ncols, st));
    HIP_TRY(fetch(s.aleatoric_var, d_noise, 1, st));
    if (int rc = wait_stream(h)) return rc;
    votes.shares(s.vote, S);
    return 0;
}

// ---- case influence (ptnn_dev_influence.hpp) ----
static_assert(PTNN_INFLUENCE_KCHUNK == INFL_KCHUNK, "ptnn.h chunk length");

int ptnn_influence(ptnn_handle* h, const ptnn_influence_spec* spec) {
    // argument checks first: none of them needs the handle or a device
    if (int rc = check_spec(spec, "ptnn_influence_spec")) return rc;
    const ptnn_influence_spec& s = *spec;
    const bool mat = s.target_values != nullptr || s.loglik != nullptr;      // source 3
    if (mat && !(s.target_values && s.loglik)) return fail(-1, "host matrices: target_values and loglik come together");
    if (mat && s.w) return fail(-1, "give host vectors w or host matrices (target_values, loglik), not both");
    const bool ll_target = s.target_kind == PTNN_INFLUENCE_LOGLIK;
    // the frame's rows are the cases; the targets are a second set of rows beside them
    RowsByVectors f(s, RowSource{s.case_source, s.case_x, s.n_cases, "case_source", "PTNN_PREDICT_X", "case_x", "n_cases"}, mat || s.w != nullptr);
    const RowSource& cases = f.rows;
    const RowSource targets{s.target_source, s.target_x, s.n_targets, "target_source", "PTNN_PREDICT_X", "target_x", "n_targets"};
    const SampleSource& src = f.src;
    if (int rc = f.check_source("target_values and loglik")) return rc;
    if (mat) {
        if (s.n_a < 1 || s.n_b < 1) return fail(-1, "n_a = %d and n_b = %d must be >= 1", s.n_a, s.n_b);
        if ((long long)s.n_a * s.n_b > PTNN_INFLUENCE_MAX_ELEMENTS)
            return fail(-1, "n_a x n_b = %d x %d: at most 2^27 elements per call", s.n_a, s.n_b);
    } else {
        if (s.target_kind != PTNN_INFLUENCE_OUTPUT && !ll_target)
            return fail(-1, "target_kind = %d is not PTNN_INFLUENCE_OUTPUT or _LOGLIK", s.target_kind);
        if (int rc = check_rows(cases)) return rc;
        if (int rc = check_rows(targets)) return rc;
        if (s.n_cases < 1 || s.n_targets < 1) return fail(-1, "n_cases = %d and n_targets = %d must be >= 1", s.n_cases, s.n_targets);
    }
    if (int rc = f.count_host()) return rc;
    if (mat)
        for (long long k = 0; k < src.n_items * s.n_b; ++k)
            if (!std::isfinite(s.loglik[k])) return fail(-1, "loglik[%lld, %lld] = %g is not finite", k / s.n_b, k % s.n_b, s.loglik[k]);
    if (int rc = check_handle(h, "ptnn_influence")) return rc;
    const int I = h->cfg.n_in, O = h->cfg.n_out;
    const bool reg = h->cfg.task == PTNN_TASK_REG;
    const int cpr = mat || ll_target ? 1 : O;                   // target columns per target row
    const long long rows_a = mat ? s.n_a : s.n_targets, n_b = mat ? s.n_b : s.n_cases, n_a = rows_a * cpr;
    if (!mat) {
        if (int rc = f.fit(h)) return rc;
        if (int rc = fit_rows(h, targets)) return rc;
        if (!reg && s.case_source == PTNN_PREDICT_X_HOST)
            if (int rc = check_labels(s.case_x, s.n_cases, I, O)) return rc;
        if (!reg && ll_target && s.target_source == PTNN_PREDICT_X_HOST)
            if (int rc = check_labels(s.target_x, s.n_targets, I, O)) return rc;
        if (n_a * n_b > PTNN_INFLUENCE_MAX_ELEMENTS)
            return fail(-1, "n_a x n_b = %lld x %lld: at most 2^27 elements per call", n_a, n_b);
    }
    if (int rc = f.select(h, s.n_samples, "a covariance (ddof 1) needs at least 2")) return rc;
    const long long M = f.M;

    // stage a: the distinct samples and their counts; every host row of source 3 is a sample of its own
    hipStream_t st = h->stream;
    DeviceScratch& mem = f.mem;
    const Distinct& d = f.d;
    const ForwardPlan& fwd = f.fwd;
    const float* d_xt = nullptr;
    int xst = 0, U = 0;
    const int* d_cnt = nullptr;
    if (mat) {
        if (int rc = f.start(h)) return rc;
        U = (int)src.n_items;
        int* cnt = nullptr;
        if (int rc = upload_counts(h, mem, s.multiplicity, (size_t)U, &cnt)) return rc;
        d_cnt = cnt;
    } else {
        f.eta = true;
        if (int rc = f.stage(h, I + 1, nullptr, [&] { return upload_rows(h, mem, targets, I + (ll_target ? 1 : 0), &d_xt, &xst); })) return rc;
        U = f.U;
        d_cnt = d.run_cnt;
        if (int rc = f.fwd.init(h, "case influence")) return rc;
    }
    const float* const d_xc = f.d_x;
    const int xsc = f.xs;
    if (s.n_distinct) *s.n_distinct = U;
    if (U > 65535LL * INFL_KCHUNK) return fail(-1, "%d distinct samples: at most 65535 x %d per call", U, INFL_KCHUNK);     // grid.y

    // The scratch: a quarter of the budget for the block of A (its double columns and, with a forward pass, its fp32 outputs), a
    // quarter for the block of B, half for the partial tiles.  Blocks are whole rows; no sum is split by them.
    const size_t budget = scratch_budget("PTNN_INFLUENCE_SCRATCH_BYTES");
    const size_t col = (size_t)U * sizeof(double), img = (size_t)U * sizeof(float) * O;
    const long long blk_a = row_block(budget / 4, mat ? col : img + col * cpr, rows_a);
    const long long blk_b = row_block(budget / 4, mat ? col : img + col, n_b);
    const int nchunks = (U + INFL_KCHUNK - 1) / INFL_KCHUNK;
    const size_t tile_bytes = (size_t)nchunks * INFL_TILE * INFL_TILE * sizeof(double);
    const auto tiles_of = [](long long n) { return (n + INFL_TILE - 1) / INFL_TILE; };
    const long long tiles_max = tiles_of(blk_a * cpr) * tiles_of(blk_b);
    const long long tiles_launch = std::max(1LL, std::min<long long>({(long long)(budget / 2 / tile_bytes), tiles_max, 65535LL}));
    double *d_A = nullptr, *d_B = nullptr, *d_part = nullptr, *d_cov = nullptr;
    double *d_ma = nullptr, *d_sa = nullptr, *d_mb = nullptr, *d_sb = nullptr;
    float* d_fx = nullptr;
    HIP_TRY(mem.alloc(&d_A, (size_t)blk_a * cpr * U));
    HIP_TRY(mem.alloc(&d_B, (size_t)blk_b * U));
    if (!mat) HIP_TRY(mem.alloc(&d_fx, (size_t)std::max(blk_a, blk_b) * O * U));
    if (s.cov) HIP_TRY(mem.alloc(&d_part, (size_t)tiles_launch * nchunks * INFL_TILE * INFL_TILE));
    if (s.cov) HIP_TRY(mem.alloc(&d_cov, (size_t)(n_a * n_b)));
    HIP_TRY(mem.alloc(&d_ma, (size_t)n_a));
    HIP_TRY(mem.alloc(&d_sa, (size_t)n_a));
    HIP_TRY(mem.alloc(&d_mb, (size_t)n_b));
    HIP_TRY(mem.alloc(&d_sb, (size_t)n_b));

    // the columns [c0, c0 + nc) of a host matrix [U][ld] as a block [nc][U] of doubles on the device
    std::vector<double> stage;
    auto host_columns = [&](auto* m, long long ld, long long c0, int nc, double* dst) -> int {
        stage.resize((size_t)nc * U);
        for (int c = 0; c < nc; ++c)
            for (int u = 0; u < U; ++u) stage[(size_t)c * U + u] = (double)m[(size_t)u * ld + c0 + c];
        HIP_TRY(hipMemcpyAsync(dst, stage.data(), stage.size() * sizeof(double), hipMemcpyHostToDevice, st));
        return wait_stream(h);                                  // `stage` is written again for the next block
    };
    ElpdRed la{};
    la.mode = reg ? ELPD_REG : ELPD_CLS; la.eta = d.run_eta; la.cnt = d_cnt; la.U = U; la.O = O; la.S = M;
    auto moments = [&](const double* v, int nc, double* mean, double* ssd) -> int {
        InflMoments ma{v, d_cnt, U, M, mean, ssd};
        HIP_TRY(launch(influence_moments_kernel, dim3((unsigned)nc), dim3(INFL_THREADS), 0, st, ma));
        return 0;
    };
    auto block_a = [&](long long r0, int nr) -> int {
        if (mat) {
            if (int rc = host_columns(s.target_values, s.n_a, r0, nr, d_A)) return rc;
        } else if (ll_target) {
            if (int rc = loglik_rows(h, fwd, d, d_xt, xst, r0, nr, d_fx, d_A, la)) return rc;
        } else {
            if (int rc = fwd.run(h, d.base, d.run_off, d_xt, xst, (int)r0, nr, U, d_fx)) return rc;
            const long long n = (long long)nr * O * U;
            HIP_TRY(launch(influence_widen_kernel, dim3((unsigned)((n + INFL_THREADS - 1) / INFL_THREADS)), dim3(INFL_THREADS), 0, st,
                           d_fx, d_A, n));
        }
        return moments(d_A, nr * cpr, d_ma + r0 * cpr, d_sa + r0 * cpr);
    };
    auto block_b = [&](long long r0, int nr) -> int {
        if (mat) {
            if (int rc = host_columns(s.loglik, s.n_b, r0, nr, d_B)) return rc;
        } else {
            if (int rc = loglik_rows(h, fwd, d, d_xc, xsc, r0, nr, d_fx, d_B, la)) return rc;
        }
        return moments(d_B, nr, d_mb + r0, d_sb + r0);
    };
    // the covariance of the two resident blocks: the tiles in launches of at most tiles_launch, each finished before the next
    auto block_cov = [&](long long ra0, int nra, long long rb0, int nrb) -> int {
        const int na = nra * cpr, tiles_b = (int)tiles_of(nrb);
        const long long tiles = tiles_of(na) * tiles_b;
        for (long long t0 = 0; t0 < tiles; t0 += tiles_launch) {
            const unsigned nt = (unsigned)std::min(tiles_launch, tiles - t0);
            InflCov ca{d_A, d_B, d_ma + ra0 * cpr, d_mb + rb0, d_cnt, na, nrb, U, tiles_b, (int)t0, nchunks, d_part};
            HIP_TRY(launch(influence_cov_kernel, dim3(nt, (unsigned)nchunks), dim3(INFL_THREADS), 0, st, ca));
            InflFinish fa{d_part, nchunks, tiles_b, (int)t0, na, nrb, n_b, (double)(M - 1), d_cov + (size_t)(ra0 * cpr) * n_b + rb0};
            HIP_TRY(launch(influence_finish_kernel, dim3(nt, INFL_TILE * INFL_TILE / INFL_THREADS), dim3(INFL_THREADS), 0, st, fa));
        }
        return 0;
    };
    // B stays resident when one block holds it; else every block of A meets every block of B, formed again (the same bits)
    const bool b_once = blk_b >= n_b;
    if (b_once || !s.cov)                                       // (without cov: the case moments alone)
        if (int rc = each_block(n_b, blk_b, block_b)) return rc;
    if (s.cov || s.target_mean || s.target_var) {
        if (int rc = each_block(rows_a, blk_a, [&](long long ra0, int nra) -> int {
            if (int rc = block_a(ra0, nra)) return rc;
            if (!s.cov) return 0;
            return each_block(n_b, blk_b, [&](long long rb0, int nrb) -> int {
                if (!b_once)
                    if (int rc = block_b(rb0, nrb)) return rc;
                return block_cov(ra0, nra, rb0, nrb);
            });
        })) return rc;
    }
    std::vector<double> ssd_a(s.target_var ? (size_t)n_a : 0), ssd_b(s.case_var ? (size_t)n_b : 0);
    HIP_TRY(fetch(s.cov, d_cov, (size_t)(n_a * n_b), st));
    HIP_TRY(fetch(s.target_mean, d_ma, (size_t)n_a, st));
    HIP_TRY(fetch(s.case_mean, d_mb, (size_t)n_b, st));
    HIP_TRY(fetch(s.target_var ? ssd_a.data() : nullptr, d_sa, (size_t)n_a, st));
    HIP_TRY(fetch(s.case_var ? ssd_b.data() : nullptr, d_sb, (size_t)n_b, st));
    if (int rc = wait_stream(h)) return rc;
    for (size_t c = 0; c < ssd_a.size(); ++c) s.target_var[c] = ssd_a[c] / (double)(M - 1);
    for (size_t c = 0; c < ssd_b.size(); ++c) s.case_var[c] = ssd_b[c] / (double)(M - 1);
    return 0;
}

// ---- posterior modes (ptnn_dev_modes.hpp) ----
int ptnn_modes(ptnn_handle* h, const ptnn_modes_spec* spec) {
    // argument checks first: none of them needs the handle or a device
    if (int rc = check_spec(spec, "ptnn_modes_spec")) return rc;
    const ptnn_modes_spec& s = *spec;
    if (s.values && s.w) return fail(-1, "give host vectors w or a host matrix values, not both");
    if (!std::isfinite(s.near_sq) || s.near_sq < 0.0) return fail(-1, "near_sq = %g must be a finite number >= 0", s.near_sq);
    SampleDistances<ptnn_modes_spec> sd(s);
    if (int rc = sd.check()) return rc;
    if (int rc = check_handle(h, "ptnn_modes")) return rc;
    if (int rc = sd.stage(h, "posterior modes")) return rc;
    hipStream_t st = h->stream;
    DeviceScratch& mem = sd.f.mem;
    const int U = sd.U;
    const int* d_cnt = sd.d_cnt;
    const long long M = sd.M;
    const bool want_parent = s.parent || s.delta_sq;
    const bool want_sq = want_parent || s.rho || s.spread_sq || s.sq_dist;
    double *d_max = nullptr, *d_part = nullptr, *d_spread = nullptr, *d_delta = nullptr;
    long long *d_rho = nullptr, *d_row_bad = nullptr, *d_bad = nullptr;
    unsigned int* d_ticket = nullptr;
    int* d_parent = nullptr;
    if (int rc = sd.alloc(want_sq)) return rc;
    const double* d_sq = sd.d_sq;
    if (want_sq) {
        HIP_TRY(mem.alloc(&d_rho, (size_t)U));
        HIP_TRY(mem.alloc(&d_max, (size_t)U));
        HIP_TRY(mem.alloc(&d_part, (size_t)U));
        HIP_TRY(mem.alloc(&d_row_bad, (size_t)U));
        HIP_TRY(mem.alloc(&d_spread, 1));
        HIP_TRY(mem.alloc(&d_bad, 2));
        HIP_TRY(mem.alloc(&d_ticket, 1));
        HIP_TRY(hipMemsetAsync(d_ticket, 0, sizeof(unsigned int), st));
    }
    if (want_parent) {
        HIP_TRY(mem.alloc(&d_parent, (size_t)U));
        HIP_TRY(mem.alloc(&d_delta, (size_t)U));
    }
    if (int rc = sd.form(h, s.item_sample != nullptr)) return rc;
    long long bad[2] = {0, -1};
    if (want_sq) {
        ModesDensity na{d_sq, d_cnt, U, s.near_sq, (double)M * (double)M, d_rho, d_max, d_part, d_row_bad, d_ticket, d_spread, d_bad};
        HIP_TRY(launch(modes_density_kernel, dim3((unsigned)U), dim3(MODES_THREADS), 0, st, na));
        if (want_parent) {
            ModesParent pa{d_sq, d_cnt, d_rho, d_max, U, d_parent, d_delta};
            HIP_TRY(launch(modes_parent_kernel, dim3((unsigned)U), dim3(MODES_THREADS), 0, st, pa));
        }
        HIP_TRY(hipMemcpyAsync(bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(fetch((long long*)s.rho, d_rho, (size_t)U, st));
    HIP_TRY(fetch(s.delta_sq, d_delta, (size_t)U, st));
    HIP_TRY(fetch((int*)s.parent, d_parent, (size_t)U, st));
    HIP_TRY(fetch(s.spread_sq, d_spread, 1, st));
    if (int rc = sd.fetch_common(st)) return rc;
    if (int rc = wait_stream(h)) return rc;
    if (bad[0] != 0)
        return fail(-1, "%lld squared distances are not finite: sample %lld is the first whose outputs are NaN or infinite", bad[0], bad[1]);
    sd.finish();
    return 0;
}

// ---- posterior compression (ptnn_dev_compress.hpp) ----
int ptnn_compress(ptnn_handle* h, const ptnn_compress_spec* spec) {
    // argument checks first: none of them needs the handle or a device
    if (int rc = check_spec(spec, "ptnn_compress_spec")) return rc;
    const ptnn_compress_spec& s = *spec;
    if (s.values && s.w) return fail(-1, "give host vectors w or a host matrix values, not both");
    if (s.m < 0) return fail(-1, "m = %d picks: must be >= 0", s.m);
    if (s.n_subsets < 0) return fail(-1, "n_subsets = %d must be >= 0", s.n_subsets);
    if (s.n_subsets > 0) {
        if (!s.subset_items) return fail(-1, "n_subsets = %d but subset_items is NULL", s.n_subsets);
        if (s.subset_size < 1 || s.subset_size > 65536) return fail(-1, "subset_size = %d outside [1, 65536]", s.subset_size);
    }
    SampleDistances<ptnn_compress_spec> sd(s);
    if (int rc = sd.check()) return rc;
    if (int rc = check_handle(h, "ptnn_compress")) return rc;
    if (int rc = sd.stage(h, "posterior compression")) return rc;
    const long long n_items = sd.f.src.n_items, n_sub = (long long)s.n_subsets * s.subset_size;
    for (long long k = 0; k < n_sub; ++k)
        if (s.subset_items[k] < 0 || s.subset_items[k] >= n_items)
            return fail(-1, "subset %lld holds item %d outside [0, %lld)", k / s.subset_size, s.subset_items[k], n_items);
    hipStream_t st = h->stream;
    DeviceScratch& mem = sd.f.mem;
    const int U = sd.U;
    const int* d_cnt = sd.d_cnt;
    // the present samples, before any further allocation: the counts are on the device since the selection
    std::vector<int> cnt((size_t)U);
    HIP_TRY(hipMemcpyAsync(cnt.data(), d_cnt, (size_t)U * sizeof(int), hipMemcpyDeviceToHost, st));
    if (int rc = wait_stream(h)) return rc;
    const long long present = (long long)std::count_if(cnt.begin(), cnt.end(), [](int c) { return c != 0; });
    if (s.m > present) return fail(-1, "m = %d picks but the selection has %lld present distinct samples", s.m, present);
    const bool want_sq = s.m > 0 || s.n_subsets > 0 || s.mu || s.d0 || s.sq_dist;
    double *d_mu = nullptr, *d_part = nullptr, *d_d0 = nullptr, *d_energy = nullptr, *d_score = nullptr, *d_sub = nullptr;
    long long *d_row_bad = nullptr, *d_bad = nullptr;
    unsigned int* d_ticket = nullptr;
    int *d_picks = nullptr, *d_items = nullptr;
    if (int rc = sd.alloc(want_sq)) return rc;
    if (want_sq) {
        HIP_TRY(mem.alloc(&d_mu, (size_t)U));
        HIP_TRY(mem.alloc(&d_part, (size_t)U));
        HIP_TRY(mem.alloc(&d_row_bad, (size_t)U));
        HIP_TRY(mem.alloc(&d_d0, 1));
        HIP_TRY(mem.alloc(&d_bad, 2));
        HIP_TRY(mem.alloc(&d_ticket, 1));
        HIP_TRY(hipMemsetAsync(d_ticket, 0, sizeof(unsigned int), st));
        HIP_TRY(mem.alloc(&d_picks, (size_t)s.m));
        HIP_TRY(mem.alloc(&d_energy, (size_t)s.m));
        HIP_TRY(mem.alloc(&d_score, (size_t)s.m));
        HIP_TRY(mem.alloc(&d_sub, (size_t)s.n_subsets));
    }
    if (int rc = sd.form(h, s.item_sample != nullptr || s.n_subsets > 0)) return rc;
    long long bad[2] = {0, -1};
    if (want_sq) {
        CompressMean ma{sd.d_sq, d_cnt, U, (double)sd.M, d_mu, d_part, d_row_bad, d_ticket, d_d0, d_bad};
        HIP_TRY(launch(compress_mean_kernel, dim3((unsigned)U), dim3(COMPRESS_THREADS), 0, st, ma));
        HIP_TRY(hipMemcpyAsync(bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, st));
        if (int rc = wait_stream(h)) return rc;                 // the items' samples are on the host now, too
        if (bad[0] != 0)
            return fail(-1, "%lld squared distances are not finite: sample %lld is the first whose outputs are NaN or infinite", bad[0], bad[1]);
    }
    if (s.n_subsets > 0) {
        for (long long k = 0; k < n_sub; ++k)
            if (cnt[(size_t)sd.sample_of(s.subset_items[k])] == 0)
                return fail(-1, "subset %lld holds item %d, whose sample %d is absent (count 0)", k / s.subset_size, s.subset_items[k],
                            sd.sample_of(s.subset_items[k]));
        HIP_TRY(mem.upload(&d_items, (const int*)s.subset_items, (size_t)n_sub, st));
        CompressSubset sa{sd.d_sq, d_mu, d_d0, sd.mat ? nullptr : sd.f.d.item_run, d_items, U, s.subset_size, d_sub};
        HIP_TRY(launch(compress_subset_kernel, dim3((unsigned)s.n_subsets), dim3(COMPRESS_THREADS), 0, st, sa));
    }
    if (s.m > 0) {
        CompressHerd ha{sd.d_sq, d_cnt, d_mu, d_d0, U, s.m, d_picks, d_energy, d_score};
        HIP_TRY(launch(compress_herd_kernel, dim3(1), dim3(COMPRESS_HERD_THREADS), 0, st, ha));
    }
    if (s.m > 0) {
        HIP_TRY(fetch((int*)s.picks, (const int*)d_picks, (size_t)s.m, st));
        HIP_TRY(fetch(s.energy, (const double*)d_energy, (size_t)s.m, st));
        HIP_TRY(fetch(s.pick_score, (const double*)d_score, (size_t)s.m, st));
    }
    HIP_TRY(fetch(s.mu, (const double*)d_mu, (size_t)U, st));
    HIP_TRY(fetch(s.d0, (const double*)d_d0, 1, st));
    if (s.n_subsets > 0) HIP_TRY(fetch(s.subset_energy, (const double*)d_sub, (size_t)s.n_subsets, st));
    if (int rc = sd.fetch_common(st)) return rc;
    if (int rc = wait_stream(h)) return rc;                     // also keeps subset_items alive until its copy is done
    sd.finish();
    return 0;
}

}  // extern "C"
