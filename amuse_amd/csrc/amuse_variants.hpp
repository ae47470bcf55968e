// The Denoiser variants behind the C ABI (include/amuse_hip.h AMUSE_ARCH_*): what amuse_api.hip forwards to amuse_variants.hip when
// a context was created with amuse_create_arch(arch != AMUSE_ARCH_ENC).
#pragma once
#include "amuse_host.hpp"
#include "amuse_pack.hpp"

size_t variant_param_count(int arch);   // floats of the variant's state dict, 0 = unknown arch
inline size_t variant_state_dim(int arch) { return (arch & 2) ? (size_t)AMUSE_POSE_STATE : (size_t)AMUSE_D_MODEL; }
// packs and uploads the variant's weight streams, parameter vectors and projection tables (first call allocates, later calls overwrite)
int variant_build(amuse_ctx* c, const float* den, int what);
void variant_destroy(amuse_ctx* c);
// after amuse_set_schedule has put timesteps / coefficients on the device: the per-step time tokens (and their K / V tables)
int variant_set_schedule(amuse_ctx* c, hipStream_t st);
int variant_sample(amuse_ctx* c, const float* con, const float* emo, const float* sty, int B, int precision, uint64_t seed,
                   uint64_t clip0, const float* x_init, const float* step_noise, float* out, float* traj_out, hipStream_t st);
// teacher-forced step: timesteps host [per_clip ? B : 1]; lengths host [B] or null (pose-space variants only)
int variant_denoise(amuse_ctx* c, const float* x_t, const int* timesteps, bool per_clip, const float* con, const float* emo,
                    const float* sty, const int* lengths, int B, int precision, float* eps_out, float* tap_out, hipStream_t st);

// ---- What amuse_api.hip and amuse_variants.hip share: the stream set of a skip network and the launch sequence "row stages + attention" that MotionPrior.decode,
// MotionPrior.encode and the pose-space Denoiser step all are.
namespace {
// which streams a skip network has (RowNet, amuse_host.hpp)
struct RowNetSpec {
    const char* blocks;            // the block stack's name in the state dict
    const float* front;            // matrix in front of stage 0, or null
    const float* back;             // matrix behind stage 9, or null
    int rows8_first, rows8_last;   // stages of the fp32x stream without split-K (first > last: none)
    bool fused16;                  // the 16-bit per-clip streams exist
    int cls;                       // AMUSE_UPD_* bits its streams need besides their precision's (AMUSE_UPD_ENCODER)
};
// packs and uploads the streams of `what`: staged x 4 precisions, rows8, per-clip fp32x, per-clip 16-bit x 2
int build_rownet_streams(amuse_ctx* c, RowNet& n, const Params& P, const RowNetSpec& sp, int what) {
    const auto wanted = [&](int prec) { return (what & (kUpdBit[prec] | sp.cls)) == (kUpdBit[prec] | sp.cls); };   // amuse_update_weights: only the requested streams are re-packed
    for (int prec = 0; prec < 4; ++prec) {
        if (!wanted(prec)) continue;
        std::vector<uint4> all;
        const auto content = [&](std::vector<uint4>& s, int st, int w) {
            if (st == 0 && sp.front) pack_in_matrix_wave(s, prec, sp.front, w);
            pack_skipnet_stage(s, prec, P, sp.blocks, st, w);
            if (st == 9 && sp.back) pack_out_matrix_wave(s, prec, sp.back, w);
        };
        if (int e = pack_staged_stream(all, n.stage_base[prec], n.stage_units[prec], content)) return e;
        if (upload(c, &n.staged[prec], all.data(), all.size() * sizeof(uint4), prec, kUpdBit[prec] | sp.cls)) return AMUSE_EHIP;
    }
    const int X = PREC_F16X2, UX = AMUSE_UPD_F32X | sp.cls;
    if (wanted(X) && sp.rows8_first <= sp.rows8_last) {   // (a matrix in front of stage 0 stays with k_vae_rows; the one behind stage 9 comes along when stage 9 does)
        std::vector<uint4> s;
        if (int e = pack_rows8_stream(s, n.rows8_base, P, sp.blocks, sp.rows8_first, sp.rows8_last, sp.rows8_last == 9 ? sp.back : nullptr)) return e;
        if (upload(c, &n.rows8, s.data(), s.size() * sizeof(uint4), X, UX)) return AMUSE_EHIP;
    }
    if (wanted(X)) {
        std::vector<uint4> s;
        if (int e = pack_fusedx_stream(s, P, sp.blocks, sp.front, sp.back)) return e;
        if (upload(c, &n.fusedx, s.data(), s.size() * sizeof(uint4), X, UX)) return AMUSE_EHIP;
    }
    for (const int p16 : {PREC_BF16, PREC_F16}) {
        if (!wanted(p16) || !sp.fused16) continue;
        std::vector<uint4> s;
        if (int e = pack_fused16_stream(s, p16, P, sp.blocks, sp.front, sp.back)) return e;
        if (upload(c, &n.fused16[p16 == PREC_F16], s.data(), s.size() * sizeof(uint4), p16, kUpdBit[p16] | sp.cls)) return AMUSE_EHIP;
    }
    return 0;
}

// host `lengths` [B] (or null: nothing to do) checked and copied to c->d_lengths.  need_full: the pose-space Denoiser's rule
int stage_lengths(amuse_ctx* c, const int* lengths, int B, bool need_full, hipStream_t st) {
    if (!lengths) return 0;
    bool full = false;
    for (int b = 0; b < B; ++b) {
        if (lengths[b] < 1 || lengths[b] > kFrames) return fail(AMUSE_EINVAL, "lengths[%d] = %d not in 1..300", b, lengths[b]);
        full |= lengths[b] == kFrames;
    }
    // lengths_to_mask sizes the mask by max(lengths) and `sample[~mask.T] = 0` needs it to be 300 (denoiser.py:145,187)
    if (need_full && !full) return fail(AMUSE_EINVAL, "max(lengths) must be 300 (the reference's mask indexing fails otherwise)");
    if (int e = ensure(&c->d_lengths, &c->len_cap, (size_t)B)) return e;
    HIP_TRY(hipMemcpyAsync(c->d_lengths, lengths, (size_t)B * sizeof(int), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

// time_tok[i] = TimestepEmbedding(ts[i]) + pe_row for n device timesteps
hipError_t time_tokens(const amuse_ctx* c, const int* ts, int n, const float* pe_row, float* out, hipStream_t st) {
    return launch_time_tokens(ts, n, c->den_freqs, c->te_w1t, c->te_b1, c->te_w2t, c->te_b2, pe_row, out, st);
}

// f(b0, nb) over a call's clips in chunks of `chunk`
template <typename F>
int for_chunks(int B, int chunk, F&& f) {
    for (int b0 = 0; b0 < B; b0 += chunk)
        if (int e = f(b0, (B - b0) < chunk ? (B - b0) : chunk)) return e;
    return 0;
}

// the staged kernels' workspace for `rows` rows: nine [rows][128] arrays (skip = 4 levels), then whatever the caller keeps behind them
struct StageWs { float *x, *q, *k, *v, *attn_o, *skip, *tail; };
StageWs carve_stage_ws(float* ws, size_t rows) {
    const size_t n = rows * kD;
    return {ws, ws + n, ws + 2 * n, ws + 3 * n, ws + 4 * n, ws + 5 * n, ws + 9 * n};
}
// arguments of one pass over the stages.  rows / attn carry the dropout tails of train-mode decode (the eval launchers take their base slice); rows8 is rows' twin
// with the stream without split-K, made by twin_rows8 once the caller has set what its network adds (outputs, lengths, tokens ...)
struct StageArgs { VaeRowsDropArgs rows; VaeRowsArgs rows8; VaeAttnDropArgs attn; };
StageArgs stage_args(const RowNet& n, int precision, const StageWs& w, int nb) {
    StageArgs a{};
    VaeRowsArgs& ra = a.rows;
    ra.wstream = n.staged[precision];
    memcpy(ra.stage_base, n.stage_base[precision], sizeof(ra.stage_base));
    memcpy(ra.stage_units, n.stage_units[precision], sizeof(ra.stage_units));
    ra.pvec = n.pvec; ra.final_bias = n.final_bias; ra.pe = n.pe; ra.emb_bias = n.emb_bias;
    ra.x = w.x; ra.q = w.q; ra.k = w.k; ra.v = w.v; ra.attn_o = w.attn_o; ra.skip = w.skip;
    ra.B = nb; ra.tiles = 19;
    a.attn.q = w.q; a.attn.k = w.k; a.attn.v = w.v; a.attn.o = w.attn_o; a.attn.B = nb; a.attn.q_tiles = 19;
    return a;
}
void twin_rows8(StageArgs& a, const RowNet& n, bool rows8) {
    a.rows8 = a.rows;
    if (rows8) {
        a.rows8.wstream = n.rows8;
        memcpy(a.rows8.stage_base, n.rows8_base, sizeof(a.rows8.stage_base));
    }
}
// stages first..9: the row kernel of `mode` - for stages r8_first..r8_last (first > last: none) launch_vae_rows8x in r8_mode on the twin - then, behind the first nine, attention
struct StageRun {
    int mode, first;
    int r8_first, r8_last, r8_mode;
    bool enc_tiles;   // MotionPrior.encode: only the distribution rows leave the last block (one tile in stage 9, one query tile in attention 8)
};
int run_stages(StageArgs& a, int precision, const StageRun& r, hipStream_t st) {
    for (int stage = r.first; stage < kVaeStages; ++stage) {
        a.rows.stage = a.rows8.stage = a.attn.layer = stage;
        if (r.enc_tiles) {
            a.rows.tiles = a.rows8.tiles = stage == kVaeStages - 1 ? 1 : 19;
            a.attn.q_tiles = stage == kLayers - 1 ? 1 : 19;
        }
        if (stage >= r.r8_first && stage <= r.r8_last) HIP_TRY(launch_vae_rows8x(a.rows8, st, r.r8_mode));
        else HIP_TRY(launch_vae_rows(a.rows, precision, r.mode, st));
        if (stage < kLayers) HIP_TRY(launch_vae_attn(a.attn, precision, r.mode, st));
    }
    return 0;
}
}  // namespace
