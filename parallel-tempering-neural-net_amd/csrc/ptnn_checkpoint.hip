// ptnn_checkpoint.hip -- ptnn_checkpoint_size / _save / _load of libptnn.so: the chain state of a handle as one buffer.
#include "ptnn_shapes.hpp"
#include "ptnn_host.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

using namespace ptnn;

extern "C" {

// ---- checkpoint / resume: the RNG is counter based, so the chain state is small and a restored handle
// continues the chains bit for bit.  Traces are not part of it: the caller keeps the rows it has fetched. ----
namespace {
struct CkHeader {
    uint32_t magic, version;
    ptnn_config cfg;
    int32_t P, PS, cur, rounds_done, finalized, have_ladder, log_rounds, reserved;
    long long counters[2];
};
constexpr uint32_t CK_MAGIC = 0x4b435450u;      // "PTCK"

// ladder adaptation (header word `reserved` = 1): the spec, both log-gap rows, the ladder history and the recorded acceptances
size_t ck_adapt_bytes(size_t R, int A, size_t logr) {
    return sizeof(ptnn_ladder_adapt_spec) + sizeof(double) * 2 * (R - 1) + sizeof(float) * ((size_t)(A + 1) * R + logr * (R - 1));
}

size_t ck_bytes(const ptnn_handle* h) {
    const size_t Rl = h->cfg.n_replicas_local, R = h->cfg.n_replicas_global, PS = h->PS;
    const size_t logr = (size_t)std::min(h->rounds_done, h->max_rounds);
    return sizeof(CkHeader) + sizeof(float) * (3 * Rl * PS + Rl * SF_COUNT + Rl + 5 * R) + sizeof(int) * (Rl + Rl * SI_COUNT + logr * R + 2 * R) +
           (h->have_adapt ? ck_adapt_bytes(R, h->adapt.rounds, logr) : 0);
}

bool same_chain(const ptnn_config& a, const ptnn_config& b) {
    return a.task == b.task && a.n_in == b.n_in && a.n_hidden == b.n_hidden && a.n_out == b.n_out &&
           a.n_replicas_local == b.n_replicas_local && a.n_replicas_global == b.n_replicas_global &&
           a.first_global_replica == b.first_global_replica && a.n_samples == b.n_samples && a.swap_interval == b.swap_interval &&
           a.pt_switch_step == b.pt_switch_step && a.use_langevin == b.use_langevin && a.swap_rule == b.swap_rule &&
           a.shared_noise == b.shared_noise && a.label_swap == b.label_swap && a.forward_bf16 == b.forward_bf16 && a.l_prob == b.l_prob &&
           a.learn_rate == b.learn_rate && a.step_w == b.step_w && a.step_eta == b.step_eta && a.sigma_squared == b.sigma_squared &&
           a.nu_1 == b.nu_1 && a.nu_2 == b.nu_2 && a.seed == b.seed;
}
}  // namespace

int ptnn_checkpoint_size(ptnn_handle* h, int64_t* bytes) {
    if (int rc = check_ready(h)) return rc;
    if (!bytes) return fail(-1, "null argument");
    *bytes = (int64_t)ck_bytes(h);
    return 0;
}

int ptnn_checkpoint_save(ptnn_handle* h, void* buf, int64_t bytes) {
    if (int rc = check_ready(h)) return rc;
    if (!buf || bytes < (int64_t)ck_bytes(h)) return fail(-1, "checkpoint buffer too small: %lld < %zu", (long long)bytes, ck_bytes(h));
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    if (int rc = finish_stream(h)) return rc;
    const size_t Rl = h->cfg.n_replicas_local, R = h->cfg.n_replicas_global, PS = h->PS;
    CkHeader hd{};
    hd.magic = CK_MAGIC; hd.version = 3; hd.cfg = h->cfg; hd.P = h->P; hd.PS = h->PS; hd.cur = h->cur;
    hd.rounds_done = h->rounds_done; hd.finalized = h->finalized ? 1 : 0; hd.have_ladder = h->have_ladder ? 1 : 0;
    hd.log_rounds = std::min(h->rounds_done, h->max_rounds);
    hd.reserved = h->have_adapt ? 1 : 0;
    HIP_TRY(hipMemcpy(hd.counters, h->d_counters, sizeof(hd.counters), hipMemcpyDeviceToHost));
    char* q = static_cast<char*>(buf);
    std::memcpy(q, &hd, sizeof(hd)); q += sizeof(hd);
    auto get = [&](const void* dev, size_t n) -> int {
        if (n) HIP_TRY(hipMemcpy(q, dev, n, hipMemcpyDeviceToHost));
        q += n;
        return 0;
    };
    if (int rc = get(h->d_state[h->flip], sizeof(float) * Rl * PS)) return rc;
    if (int rc = get(h->d_gd_w[h->flip], sizeof(float) * Rl * PS)) return rc;
    if (int rc = get(h->d_rec_w, sizeof(float) * Rl * PS)) return rc;
    if (int rc = get(h->d_st_f, sizeof(float) * Rl * SF_COUNT)) return rc;
    if (int rc = get(h->d_temps, sizeof(float) * Rl)) return rc;
    if (int rc = get(h->d_L_handoff, sizeof(float) * R)) return rc;
    if (int rc = get(h->d_L_final, sizeof(float) * R)) return rc;
    if (int rc = get(h->d_L_raw, sizeof(float) * R)) return rc;
    if (int rc = get(h->d_prior_post, sizeof(float) * R)) return rc;
    if (int rc = get(h->d_temps_global, sizeof(float) * R)) return rc;
    if (int rc = get(h->d_gd_valid[h->flip], sizeof(int) * Rl)) return rc;
    if (int rc = get(h->d_st_i, sizeof(int) * Rl * SI_COUNT)) return rc;
    if (int rc = get(h->d_src_log, sizeof(int) * (size_t)hd.log_rounds * R)) return rc;
    if (int rc = get(h->d_label[h->lflip], sizeof(int) * R)) return rc;          // slot <-> temperature maps (identity unless label_swap)
    if (int rc = get(h->d_slot_of[h->lflip], sizeof(int) * R)) return rc;
    if (h->have_adapt) {
        std::memcpy(q, &h->adapt, sizeof(h->adapt)); q += sizeof(h->adapt);
        if (int rc = get(h->d_lad_s, sizeof(double) * 2 * (R - 1))) return rc;
        if (int rc = get(h->d_lad_hist, sizeof(float) * (size_t)(h->adapt.rounds + 1) * R)) return rc;
        if (int rc = get(h->d_lad_acc, sizeof(float) * (size_t)hd.log_rounds * (R - 1))) return rc;
    }
    return 0;
}

int ptnn_checkpoint_load(ptnn_handle* h, const void* buf, int64_t bytes) {
    if (!h || !buf) return fail(-1, "null argument");
    if (!h->have_data) return fail(-1, "call ptnn_set_data before ptnn_checkpoint_load");
    if (bytes < (int64_t)sizeof(CkHeader)) return fail(-1, "not a checkpoint (too short)");
    CkHeader hd;
    std::memcpy(&hd, buf, sizeof(hd));
    if (hd.magic != CK_MAGIC || hd.version != 3) return fail(-1, "not a libptnn checkpoint (magic %08x version %u)", hd.magic, hd.version);
    if (!same_chain(hd.cfg, h->cfg) || hd.P != h->P || hd.PS != h->PS)
        return fail(-1, "the checkpoint was written by chains with a different configuration (topology, replicas, samples, seed ...)");
    HIP_TRY(hipSetDevice(h->cfg.device_id));
    if (int rc = wait_stream(h)) return rc;
    const size_t Rl = h->cfg.n_replicas_local, R = h->cfg.n_replicas_global, PS = h->PS;
    const size_t need = sizeof(CkHeader) + sizeof(float) * (3 * Rl * PS + Rl * SF_COUNT + Rl + 5 * R) +
                        sizeof(int) * (Rl + Rl * SI_COUNT + (size_t)hd.log_rounds * R + 2 * R);
    if ((size_t)bytes < need) return fail(-1, "truncated checkpoint: %lld < %zu bytes", (long long)bytes, need);
    if (hd.log_rounds > h->max_rounds) return fail(-1, "checkpoint holds more swap rounds than this handle can log");
    if (hd.reserved != 0 && hd.reserved != 1) return fail(-1, "not a libptnn checkpoint (unknown trailer %d)", hd.reserved);
    ptnn_ladder_adapt_spec ad{};
    if (hd.reserved == 1) {
        if ((size_t)bytes < need + sizeof(ad)) return fail(-1, "truncated checkpoint: no ladder adaptation spec");
        std::memcpy(&ad, static_cast<const char*>(buf) + need, sizeof(ad));
        if (ad.struct_bytes != (int32_t)sizeof(ad) || ad.rounds < 0 || ad.rounds > h->max_rounds)
            return fail(-1, "the checkpoint's ladder adaptation spec is not valid here");
        if (h->have_adapt && (h->adapt.rounds != ad.rounds || h->adapt.kappa0 != ad.kappa0 || h->adapt.t0 != ad.t0))
            return fail(-1, "the checkpoint adapts the ladder over %d rounds (kappa0 %g, t0 %g), this handle over %d (kappa0 %g, t0 %g): "
                            "set the same adaptation, or none, before loading it", ad.rounds, ad.kappa0, ad.t0, h->adapt.rounds,
                        h->adapt.kappa0, h->adapt.t0);
        const size_t full = need + ck_adapt_bytes(R, ad.rounds, (size_t)hd.log_rounds);
        if ((size_t)bytes < full) return fail(-1, "truncated checkpoint: %lld < %zu bytes", (long long)bytes, full);
    } else if (h->have_adapt) {
        return fail(-1, "the checkpoint was written without ladder adaptation, this handle adapts the ladder: clear it first "
                        "(ptnn_set_ladder)");
    }
    const char* q = static_cast<const char*>(buf) + sizeof(CkHeader);
    auto put = [&](void* dev, size_t n) -> int {
        if (n) HIP_TRY(hipMemcpy(dev, q, n, hipMemcpyHostToDevice));
        q += n;
        return 0;
    };
    h->flip = 0;
    if (int rc = put(h->d_state[0], sizeof(float) * Rl * PS)) return rc;
    if (int rc = put(h->d_gd_w[0], sizeof(float) * Rl * PS)) return rc;
    if (int rc = put(h->d_rec_w, sizeof(float) * Rl * PS)) return rc;
    if (int rc = put(h->d_st_f, sizeof(float) * Rl * SF_COUNT)) return rc;
    if (int rc = put(h->d_temps, sizeof(float) * Rl)) return rc;
    if (int rc = put(h->d_L_handoff, sizeof(float) * R)) return rc;
    if (int rc = put(h->d_L_final, sizeof(float) * R)) return rc;
    if (int rc = put(h->d_L_raw, sizeof(float) * R)) return rc;
    if (int rc = put(h->d_prior_post, sizeof(float) * R)) return rc;
    if (int rc = put(h->d_temps_global, sizeof(float) * R)) return rc;
    if (int rc = put(h->d_gd_valid[0], sizeof(int) * Rl)) return rc;
    if (int rc = put(h->d_st_i, sizeof(int) * Rl * SI_COUNT)) return rc;
    if (int rc = put(h->d_src_log, sizeof(int) * (size_t)hd.log_rounds * R)) return rc;
    h->lflip = 0;
    if (int rc = put(h->d_label[0], sizeof(int) * R)) return rc;
    if (int rc = put(h->d_slot_of[0], sizeof(int) * R)) return rc;
    if (hd.reserved == 1) {
        // the adaptation travels with the chains: spec, log-gaps and both records as they were
        if (int rc = ladder_adapt_alloc(h, ad)) return rc;
        q += sizeof(ad);
        if (int rc = put(h->d_lad_s, sizeof(double) * 2 * (R - 1))) return rc;
        if (int rc = put(h->d_lad_hist, sizeof(float) * (size_t)(ad.rounds + 1) * R)) return rc;
        HIP_TRY(hipMemset(h->d_lad_acc, 0xff, (size_t)h->max_rounds * (R - 1) * sizeof(float)));
        if (int rc = put(h->d_lad_acc, sizeof(float) * (size_t)hd.log_rounds * (R - 1))) return rc;
        // a restart of this handle (ptnn_set_state) starts from the checkpoint's initial ladder, row 0 of its history
        h->lad_T0.resize(R);
        HIP_TRY(hipMemcpy(h->lad_T0.data(), h->d_lad_hist, R * sizeof(float), hipMemcpyDeviceToHost));
        h->lad_s0.resize(R - 1);
        for (size_t k = 0; k + 1 < R; ++k) h->lad_s0[k] = std::log((double)h->lad_T0[k + 1] - (double)h->lad_T0[k]);
    }
    HIP_TRY(hipMemcpy(h->d_state[1], h->d_state[0], sizeof(float) * Rl * PS, hipMemcpyDeviceToDevice));
    if (h->plan.compact) {
        // compact traces: the rows a later rejected step may repeat are not on this device -- put the recorded row of every chain
        // into trace row hd.cur (the last one before the checkpoint) and point the chains at it
        HIP_TRY(hipMemcpy2D(h->d_pos_w + (size_t)(hd.cur % h->cap) * h->PW, (size_t)h->cap * h->PW * sizeof(float), h->d_rec_w,
                            PS * sizeof(float), (size_t)h->P * sizeof(float), Rl, hipMemcpyDeviceToDevice));
        std::vector<int> si(Rl * SI_COUNT);
        HIP_TRY(hipMemcpy(si.data(), h->d_st_i, si.size() * sizeof(int), hipMemcpyDeviceToHost));
        for (size_t r = 0; r < Rl; ++r) si[r * SI_COUNT + SI_REC_ROW] = hd.cur;
        HIP_TRY(hipMemcpy(h->d_st_i, si.data(), si.size() * sizeof(int), hipMemcpyHostToDevice));
    }
    HIP_TRY(hipMemcpy(h->d_counters, hd.counters, sizeof(hd.counters), hipMemcpyHostToDevice));
    h->cur = hd.cur; h->rounds_done = hd.rounds_done; h->finalized = hd.finalized != 0; h->have_ladder = hd.have_ladder != 0;
    h->drained = hd.cur; h->first_row = hd.cur + 1;
    HIP_TRY(hipMemset(h->d_error, 0, sizeof(int)));
    if (!h->comm.failed) { h->failed = false; h->failure.clear(); }
    h->h_progress[0] = h->h_progress[1] = hd.rounds_done;
    h->have_state = true;
    return 0;
}

}  // extern "C"
