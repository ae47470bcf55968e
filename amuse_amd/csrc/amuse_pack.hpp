// Host-side weight packing of the library (amuse_api.hip, amuse_variants.hip - no kernel translation unit includes this): the state-dict index, the MFMA-fragment
// unit packer (amuse_dev.hpp has the device side of the unit layout) and ONE packer per weight-stream layout.  A layout's order is stated here once, next to
// the name of the kernel that consumes it; the builders (build_denoiser, build_prior, variant_build) say which parameters, precision and front / back
// matrices go into it.  amuse_update_weights runs all of this once per training iteration: plain functions and templates on a callable, appending to the
// caller's vector - no std::function, no virtual call, no intermediate copy of a stream.
#pragma once
#include "amuse_host.hpp"

namespace {
// ---------------------------------------------------------------- state-dict index (order = reference)
struct ParamIndex {
    std::map<std::string, std::pair<size_t, size_t>> m;  // name -> (offset, numel)
    size_t total = 0;
    void add(const std::string& n, size_t numel) { m[n] = {total, numel}; total += numel; }
};

void enc_layer(ParamIndex& P, const std::string& p) {
    P.add(p + ".self_attn.in_proj_weight", 384 * 128); P.add(p + ".self_attn.in_proj_bias", 384);
    P.add(p + ".self_attn.out_proj.weight", 128 * 128); P.add(p + ".self_attn.out_proj.bias", 128);
    P.add(p + ".linear1.weight", 512 * 128); P.add(p + ".linear1.bias", 512);
    P.add(p + ".linear2.weight", 128 * 512); P.add(p + ".linear2.bias", 128);
    P.add(p + ".norm1.weight", 128); P.add(p + ".norm1.bias", 128);
    P.add(p + ".norm2.weight", 128); P.add(p + ".norm2.bias", 128);
}
void dec_layer(ParamIndex& P, const std::string& p) {
    P.add(p + ".self_attn.in_proj_weight", 384 * 128); P.add(p + ".self_attn.in_proj_bias", 384);
    P.add(p + ".self_attn.out_proj.weight", 128 * 128); P.add(p + ".self_attn.out_proj.bias", 128);
    P.add(p + ".multihead_attn.in_proj_weight", 384 * 128); P.add(p + ".multihead_attn.in_proj_bias", 384);
    P.add(p + ".multihead_attn.out_proj.weight", 128 * 128); P.add(p + ".multihead_attn.out_proj.bias", 128);
    P.add(p + ".linear1.weight", 512 * 128); P.add(p + ".linear1.bias", 512);
    P.add(p + ".linear2.weight", 128 * 512); P.add(p + ".linear2.bias", 128);
    for (const char* n : {"norm1", "norm2", "norm3"}) { P.add(p + "." + n + ".weight", 128); P.add(p + "." + n + ".bias", 128); }
}
std::string blk_name(const std::string& prefix, int blk) {
    if (blk < 4) return prefix + ".input_blocks." + std::to_string(blk);
    if (blk == 4) return prefix + ".middle_block";
    return prefix + ".output_blocks." + std::to_string(blk - 5);
}
void skip_stack(ParamIndex& P, const std::string& prefix, bool dec) {
    P.add(prefix + ".norm.weight", 128); P.add(prefix + ".norm.bias", 128);
    for (int b = 0; b < 9; ++b) dec ? dec_layer(P, blk_name(prefix, b)) : enc_layer(P, blk_name(prefix, b));
    for (int i = 0; i < 4; ++i) {
        P.add(prefix + ".linear_blocks." + std::to_string(i) + ".weight", 128 * 256);
        P.add(prefix + ".linear_blocks." + std::to_string(i) + ".bias", 128);
    }
}
ParamIndex denoiser_index() {
    ParamIndex P;
    P.add("time_embedding.linear_1.weight", 128 * 256); P.add("time_embedding.linear_1.bias", 128);
    P.add("time_embedding.linear_2.weight", 128 * 128); P.add("time_embedding.linear_2.bias", 128);
    for (const char* n : {"con", "emo", "sty"}) {
        P.add(std::string("emb_proj_") + n + ".1.weight", 128 * 256);
        P.add(std::string("emb_proj_") + n + ".1.bias", 128);
    }
    P.add("query_pos.pe", 500 * 128); P.add("mem_pos.pe", 500 * 128);
    skip_stack(P, "encoder", false);
    return P;
}
ParamIndex prior_index() {
    ParamIndex P;
    P.add("global_motion_token", 2 * 128);
    P.add("query_pos_encoder.pe", 500 * 128); P.add("query_pos_decoder.pe", 500 * 128);
    skip_stack(P, "encoder", false);
    skip_stack(P, "decoder", true);
    P.add("skel_embedding.weight", 128 * 333); P.add("skel_embedding.bias", 128);
    P.add("final_layer.weight", 333 * 128); P.add("final_layer.bias", 333);
    return P;
}
struct Params {
    const ParamIndex& idx;
    const float* base;
    const float* get(const std::string& n) const { return base + idx.m.at(n).first; }
};

// ---------------------------------------------------------------- MFMA-fragment packing (see amuse_dev.hpp)
uint16_t f2bf(float f) {  // round-to-nearest-even, as v_cvt_pk_bf16_f32
    uint32_t x;
    memcpy(&x, &f, 4);
    if ((x & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((x >> 16) | 0x40);
    x += 0x7fffu + ((x >> 16) & 1u);
    return (uint16_t)(x >> 16);
}
// fp32 -> fp16 bits, round-to-nearest-even with gradual underflow (what v_cvt_pk_f16_f32 / (_Float16) do), and back (exact)
uint16_t f2h(float f) {
    uint32_t x;
    memcpy(&x, &f, 4);
    const uint16_t sign = (uint16_t)((x >> 16) & 0x8000u);
    x &= 0x7fffffffu;
    if (x > 0x7f800000u) return (uint16_t)(sign | 0x7e00u);          // NaN
    if (x >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);         // >= 65520 rounds to infinity
    if (x < 0x38800000u) {                                            // below 2^-14: the result is subnormal (or 2^-14)
        float a;
        memcpy(&a, &x, 4);
        return (uint16_t)(sign | (uint16_t)nearbyintf(a * 16777216.0f));   // units of 2^-24, ties to even
    }
    x -= 0x38000000u;                                                 // re-bias the exponent (127 -> 15)
    x += 0xfffu + ((x >> 13) & 1u);
    return (uint16_t)(sign | (x >> 13));
}
float h2f(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3ffu;
    float f;
    if (e == 0) {
        f = (float)m * 5.9604644775390625e-8f;                        // m * 2^-24
        uint32_t u;
        memcpy(&u, &f, 4);
        u |= sign;
        memcpy(&f, &u, 4);
        return f;
    }
    const uint32_t u = sign | (e == 31 ? 0x7f800000u | (m << 13) : ((e + 112u) << 23) | (m << 13));
    memcpy(&f, &u, 4);
    return f;
}
// W: [n_out x K] row-major.  Appends units for (k-tile outer, out-tile inner); PREC_F16X2: k-tile pair outer, out-tile inner,
// two units each - hi = rn16(w), lo = rn16(w - hi) (amuse_dev.hpp gemm_ring_s).
void pack_gemm(std::vector<uint4>& out, int prec, const float* W, int n_out, int K, const std::vector<int>& otiles,
               const std::vector<int>& ktiles) {
    // (amuse_update_weights calls this once per training iteration: the destination is sized once and filled through a
    // pointer, rows / columns inside the matrix skip the bounds checks)
    const size_t nunits = is_op16(prec) ? (ktiles.size() / 2) * otiles.size() : ktiles.size() * otiles.size();
    uint16_t (*const cv16)(float) = prec == PREC_F16 ? f2h : f2bf;   // the one-piece 16-bit formats differ in the conversion only
    const size_t base = out.size();
    out.resize(base + nunits * 64);
    uint4* dst = out.data() + base;
    auto at = [&](int row, int col) -> float { return (row < n_out && col < K) ? W[(size_t)row * K + col] : 0.f; };
    if (prec == PREC_F32) {
        for (int t : ktiles)
            for (int o : otiles) {
                const bool inside = 16 * o + 16 <= n_out && 16 * t + 16 <= K;
                for (int lane = 0; lane < 64; ++lane, ++dst) {
                    const int g = lane >> 4, i = lane & 15;
                    float v[4];
                    if (inside) memcpy(v, W + (size_t)(16 * o + i) * K + 16 * t + 4 * g, 16);
                    else
                        for (int m = 0; m < 4; ++m) v[m] = at(16 * o + i, 16 * t + 4 * g + m);
                    memcpy(dst, v, 16);
                }
            }
    } else if (prec == PREC_F16X2) {
        for (size_t c = 0; c + 1 < ktiles.size(); c += 2) {
            const int t0 = ktiles[c], t1 = ktiles[c + 1];
            for (int o : otiles) {
                for (int lane = 0; lane < 64; ++lane, ++dst) {
                    const int g = lane >> 4, i = lane & 15;
                    uint16_t hi[8], lo[8];
                    for (int e = 0; e < 8; ++e) {
                        const float w = at(16 * o + i, 16 * (e < 4 ? t0 : t1) + 4 * g + (e & 3));
                        hi[e] = f2h(w);
                        lo[e] = g_probe_f16 ? hi[e] : f2h(w - h2f(hi[e]));
                    }
                    memcpy(dst, hi, 16);
                    memcpy(dst + 64, lo, 16);
                }
                dst += 64;
            }
        }
    } else {
        for (size_t c = 0; c + 1 < ktiles.size(); c += 2) {
            const int t0 = ktiles[c], t1 = ktiles[c + 1];
            for (int o : otiles) {
                const bool inside = 16 * o + 16 <= n_out && 16 * t0 + 16 <= K && 16 * t1 + 16 <= K;
                for (int lane = 0; lane < 64; ++lane, ++dst) {
                    const int g = lane >> 4, i = lane & 15;
                    uint16_t v[8];
                    if (inside) {
                        const float* r0 = W + (size_t)(16 * o + i) * K + 16 * t0 + 4 * g;
                        const float* r1 = W + (size_t)(16 * o + i) * K + 16 * t1 + 4 * g;
                        for (int e = 0; e < 4; ++e) { v[e] = cv16(r0[e]); v[4 + e] = cv16(r1[e]); }
                    } else {
                        for (int e = 0; e < 4; ++e) {
                            v[e] = cv16(at(16 * o + i, 16 * t0 + 4 * g + e));
                            v[4 + e] = cv16(at(16 * o + i, 16 * t1 + 4 * g + e));
                        }
                    }
                    memcpy(dst, v, 16);
                }
            }
        }
    }
}
std::vector<int> range(int a, int b) { std::vector<int> r; for (int i = a; i < b; ++i) r.push_back(i); return r; }

void fill_block_pvec(float* pv, const Params& P, const std::string& p, bool dec) {
    memcpy(pv + PV_IN_B, P.get(p + ".self_attn.in_proj_bias"), 384 * 4);
    memcpy(pv + PV_OUT_B, P.get(p + ".self_attn.out_proj.bias"), 128 * 4);
    memcpy(pv + PV_L1_B, P.get(p + ".linear1.bias"), 512 * 4);
    memcpy(pv + PV_L2_B, P.get(p + ".linear2.bias"), 128 * 4);
    memcpy(pv + PV_LN1_W, P.get(p + ".norm1.weight"), 128 * 4); memcpy(pv + PV_LN1_B, P.get(p + ".norm1.bias"), 128 * 4);
    memcpy(pv + PV_LN2_W, P.get(p + ".norm2.weight"), 128 * 4); memcpy(pv + PV_LN2_B, P.get(p + ".norm2.bias"), 128 * 4);
    if (dec) { memcpy(pv + PV_LN3_W, P.get(p + ".norm3.weight"), 128 * 4); memcpy(pv + PV_LN3_B, P.get(p + ".norm3.bias"), 128 * 4); }
}
std::vector<float> build_pvec(const Params& P, const std::string& prefix, bool dec) {
    std::vector<float> pv(PV_TOTAL, 0.f);
    for (int b = 0; b < 9; ++b) fill_block_pvec(pv.data() + b * PV_BLOCK, P, blk_name(prefix, b), dec);
    for (int i = 0; i < 4; ++i)
        memcpy(pv.data() + PV_SKIP_B + i * 128, P.get(prefix + ".linear_blocks." + std::to_string(i) + ".bias"), 128 * 4);
    memcpy(pv.data() + PV_FINAL_W, P.get(prefix + ".norm.weight"), 128 * 4);
    memcpy(pv.data() + PV_FINAL_B, P.get(prefix + ".norm.bias"), 128 * 4);
    return pv;
}
// the per-wave pieces shared by encoder and decoder blocks
void pack_qkv(std::vector<uint4>& s, int prec, const float* in_w, int h, bool v_separate) {
    if (v_separate) {  // sampler: q,k tiles as one 4-tile GEMM, then v (operand-swapped on the device)
        pack_gemm(s, prec, in_w, 384, 128, {2 * h, 2 * h + 1, 8 + 2 * h, 8 + 2 * h + 1}, range(0, 8));
        pack_gemm(s, prec, in_w, 384, 128, {16 + 2 * h, 16 + 2 * h + 1}, range(0, 8));
    } else {
        pack_gemm(s, prec, in_w, 384, 128, {2 * h, 2 * h + 1, 8 + 2 * h, 8 + 2 * h + 1, 16 + 2 * h, 16 + 2 * h + 1}, range(0, 8));
    }
}
void pack_outproj_ffn(std::vector<uint4>& s, int prec, const Params& P, const std::string& p, int w) {
    pack_gemm(s, prec, P.get(p + ".self_attn.out_proj.weight"), 128, 128, range(0, 8), {2 * w, 2 * w + 1});
    pack_gemm(s, prec, P.get(p + ".linear1.weight"), 512, 128, range(8 * w, 8 * w + 8), range(0, 8));
    pack_gemm(s, prec, P.get(p + ".linear2.weight"), 128, 512, range(0, 8), range(8 * w, 8 * w + 8));
}
// sampler order: out_proj, then the FFN in four software-pipelined quarters (k_sampler.hip encoder_block)
void pack_outproj_ffn_quarters(std::vector<uint4>& s, int prec, const Params& P, const std::string& p, int w) {
    pack_gemm(s, prec, P.get(p + ".self_attn.out_proj.weight"), 128, 128, range(0, 8), {2 * w, 2 * w + 1});
    // software-pipelined order of k_sampler.hip: F1q0 F1q1 F2q0 F1q2 F2q1 F1q3 F2q2 F2q3
    auto f1 = [&](int q) { const int h0 = 8 * w + 2 * q; pack_gemm(s, prec, P.get(p + ".linear1.weight"), 512, 128, {h0, h0 + 1}, range(0, 8)); };
    auto f2 = [&](int q) { const int h0 = 8 * w + 2 * q; pack_gemm(s, prec, P.get(p + ".linear2.weight"), 128, 512, range(0, 8), {h0, h0 + 1}); };
    f1(0); f1(1); f2(0); f1(2); f2(1); f1(3); f2(2); f2(3);
}
void pack_skiplin(std::vector<uint4>& s, int prec, const Params& P, const std::string& prefix, int i, int w) {
    pack_gemm(s, prec, P.get(prefix + ".linear_blocks." + std::to_string(i) + ".weight"), 128, 256, range(0, 8),
              range(4 * w, 4 * w + 4));
}
std::vector<float> transpose(const float* w, int rows, int cols) {  // [rows][cols] -> [cols][rows]
    std::vector<float> t((size_t)rows * cols);
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) t[(size_t)c * rows + r] = w[(size_t)r * cols + c];
    return t;
}
// what every Denoiser arch has beside its transformer: the time-embedding MLP and the three condition projections, transposed for the prologue kernels (k_misc.hip)
int upload_embeddings(amuse_ctx* c, const Params& D) {
    const auto w1t = transpose(D.get("time_embedding.linear_1.weight"), 128, 256);
    const auto w2t = transpose(D.get("time_embedding.linear_2.weight"), 128, 128);
    if (upload(c, &c->te_w1t, w1t.data(), w1t.size() * 4) || upload(c, &c->te_w2t, w2t.data(), w2t.size() * 4) ||
        upload(c, &c->te_b1, D.get("time_embedding.linear_1.bias"), 512) || upload(c, &c->te_b2, D.get("time_embedding.linear_2.bias"), 512))
        return AMUSE_EHIP;
    const char* names[3] = {"con", "emo", "sty"};
    for (int n = 0; n < 3; ++n) {
        const std::string p = std::string("emb_proj_") + names[n] + ".1";
        const auto wt = transpose(D.get(p + ".weight"), 128, 256);
        if (upload(c, &c->cond_wt[n], wt.data(), wt.size() * 4) || upload(c, &c->cond_b[n], D.get(p + ".bias"), 512)) return AMUSE_EHIP;
    }
    return 0;
}

// ---------------------------------------------------------------- the stream layouts, one packer each
constexpr size_t kUnit = 64;   // uint4 per 1 KiB unit
void pad_units(std::vector<uint4>& s, size_t units) { s.insert(s.end(), units * kUnit, uint4{0, 0, 0, 0}); }
// the four matrices of a transformer block's self-attention + FFN, and the pieces several layouts cut them into
struct BlockW { const float *in_w, *out_w, *l1, *l2; };
BlockW block_w(const Params& P, const std::string& p) {
    return {P.get(p + ".self_attn.in_proj_weight"), P.get(p + ".self_attn.out_proj.weight"), P.get(p + ".linear1.weight"), P.get(p + ".linear2.weight")};
}
const float* skip_w(const Params& P, const std::string& prefix, int i) { return P.get(prefix + ".linear_blocks." + std::to_string(i) + ".weight"); }
// FFN slices of `n` tiles of the hidden dimension from tile t0: linear1's output tiles / linear2's k-tiles
void pack_f1(std::vector<uint4>& s, int prec, const BlockW& W, int t0, int n) { pack_gemm(s, prec, W.l1, 512, 128, range(t0, t0 + n), range(0, 8)); }
void pack_f2(std::vector<uint4>& s, int prec, const BlockW& W, int t0, int n) { pack_gemm(s, prec, W.l2, 128, 512, range(0, 8), range(t0, t0 + n)); }
// the skip linear on cat(x, skip) for all eight output tiles: the x half (k-tiles 0..7), then the popped-skip half
void pack_skip_halves(std::vector<uint4>& s, int prec, const float* wskip) {
    pack_gemm(s, prec, wskip, 128, 256, range(0, 8), range(0, 8));
    pack_gemm(s, prec, wskip, 128, 256, range(0, 8), range(8, 16));
}
// one head's k | v tiles per k-pair, then its q tiles (the per-clip kernels project K / V of a head, then Q)
void pack_head_kv_q(std::vector<uint4>& s, int prec, const float* in_w, int h) {
    pack_gemm(s, prec, in_w, 384, 128, {8 + 2 * h, 8 + 2 * h + 1, 16 + 2 * h, 16 + 2 * h + 1}, range(0, 8));
    pack_gemm(s, prec, in_w, 384, 128, {2 * h, 2 * h + 1}, range(0, 8));
}
// a [kFeats][128] output matrix (final_layer / pose_proj; 24 output tiles, the last three padding) in `parts` groups of 24 / parts tiles
void pack_out_matrix(std::vector<uint4>& s, int prec, const float* w, int parts) {
    const int n = kFeatTiles / parts;
    for (int q = 0; q < parts; ++q) pack_gemm(s, prec, w, kFeats, 128, range(n * q, n * q + n), range(0, 8));
}
// a [128][kFeats] input embedding (skel_embedding / pose_embd; K = 333 padded to 22 k-tiles) for all eight output tiles
void pack_in_matrix(std::vector<uint4>& s, int prec, const float* w) { pack_gemm(s, prec, w, 128, kFeats, range(0, 8), range(0, 22)); }
int whole_stages(const std::vector<uint4>& s, size_t stage_units, const char* what) {
    return s.size() % (stage_units * kUnit) == 0 ? 0 : fail(AMUSE_ESTATE, "internal: %s stream is not whole stages", what);
}

// fp32x per-clip stream (k_vae_fusedx.hip: k_vae_fusedx, k_den_fusedx): ONE stream of unit pairs (hi | lo) for the clip's eight waves in consumption order, 16-unit
// stages.  [front: the input embedding, 11 k-pairs x 8 output tiles] | nine blocks: [skip linear ahead of an output block: x half, popped-skip half] | per head
// k | v (two stages) then q (one stage) | out_proj | the FFN in 16 chunks of 32 hidden features with linear1 one chunk ahead: f1(0), 15 x [f1(ch + 1), f2(ch)],
// f2(15) | [back: the output matrix in four quarters of six tiles] | two stages of padding (the fetch runs two stages ahead).
int pack_fusedx_stream(std::vector<uint4>& s, const Params& P, const std::string& prefix, const float* front, const float* back) {
    constexpr int X = PREC_F16X2;
    if (front) pack_in_matrix(s, X, front);
    for (int b = 0; b < 9; ++b) {
        const BlockW W = block_w(P, blk_name(prefix, b));
        if (b >= 5) pack_skip_halves(s, X, skip_w(P, prefix, b - 5));
        for (int h = 0; h < 4; ++h) pack_head_kv_q(s, X, W.in_w, h);
        pack_gemm(s, X, W.out_w, 128, 128, range(0, 8), range(0, 8));
        const auto f1 = [&](int ch) { pack_f1(s, X, W, 2 * ch, 2); };
        const auto f2 = [&](int ch) { pack_f2(s, X, W, 2 * ch, 2); };
        f1(0);
        for (int ch = 0; ch < 15; ++ch) { f1(ch + 1); f2(ch); }
        f2(15);
    }
    if (back) pack_out_matrix(s, X, back, 4);
    if (int e = whole_stages(s, 16, "fused fp32x")) return e;
    pad_units(s, 2 * 16);
    return 0;
}

// 16-bit fused per-clip stream (k_vae_fused.hip, k_den_fused.hip; bf16 / fp16 operands): ONE stream in consumption order, cut into stages of kVaeFusedStageUnits
// units - every phase is a whole number of stages.  [front: the input embedding | pad(8)] | nine blocks: [skip linear: x half, popped-skip half] | per head:
// stage A = k | v tiles per k-pair, stage B = q, out_proj's k-slice | the FFN software-pipelined: [f1(0) | pad(8)], 15 x [f1(ch + 1) | f2(ch)], [f2(15) | pad(8)] |
// back: the output matrix ONCE in two halves of 48 units (the kernel's last stage holds it in LDS whole) | two stages of padding (the fetch runs two ahead).
int pack_fused16_stream(std::vector<uint4>& s, int p16, const Params& P, const std::string& prefix, const float* front, const float* back) {
    if (front) { pack_in_matrix(s, p16, front); pad_units(s, 8); }
    for (int b = 0; b < 9; ++b) {
        const BlockW W = block_w(P, blk_name(prefix, b));
        if (b >= 5) pack_skip_halves(s, p16, skip_w(P, prefix, b - 5));
        for (int h = 0; h < 4; ++h) {
            pack_head_kv_q(s, p16, W.in_w, h);
            pack_gemm(s, p16, W.out_w, 128, 128, range(0, 8), {2 * h, 2 * h + 1});
        }
        const auto f1 = [&](int ch) { pack_f1(s, p16, W, 2 * ch, 2); };
        const auto f2 = [&](int ch) { pack_f2(s, p16, W, 2 * ch, 2); };
        f1(0); pad_units(s, 8);
        for (int ch = 0; ch < 15; ++ch) { f1(ch + 1); f2(ch); }
        f2(15); pad_units(s, 8);
    }
    pack_out_matrix(s, p16, back, 2);
    if (int e = whole_stages(s, kVaeFusedStageUnits, "fused 16-bit")) return e;
    pad_units(s, 2 * kVaeFusedStageUnits);
    return 0;
}

// fp32x row stages without split-K, eight tiles per workgroup (k_vae_rows8.hip): per stage ONE stream in consumption order, in 16-unit (8 hi | lo pairs) LDS
// stages - each one k-pair x 8 output tiles or, for linear1, 4 k-pairs x 2 output tiles.  Stage st >= 1 = what follows block st - 1's attention: out_proj |
// 16 x [linear1 chunk, linear2 chunk] | [blocks 4..7: the skip linear ahead of output block st: x half, popped-skip half]; then the next block's in_proj in three
// groups of eight tiles (q | k | v) or, in stage 9 with `back`, the output matrix in quarters.  Stages outside [first, last] stay with k_vae_rows (their base is
// recorded, they hold nothing); two stages of padding behind the last (the fetch runs two ahead).
int pack_rows8_stream(std::vector<uint4>& s, uint32_t* base, const Params& P, const std::string& prefix, int first, int last, const float* back) {
    constexpr int X = PREC_F16X2;
    for (int st = 0; st < kVaeStages; ++st) {
        base[st] = (uint32_t)(s.size() / kUnit);
        if (st < first || st > last) continue;
        if (st >= 1) {
            const int b = st - 1;
            const BlockW W = block_w(P, blk_name(prefix, b));
            pack_gemm(s, X, W.out_w, 128, 128, range(0, 8), range(0, 8));
            for (int ch = 0; ch < 16; ++ch) { pack_f1(s, X, W, 2 * ch, 2); pack_f2(s, X, W, 2 * ch, 2); }
            if (b >= 4 && b <= 7) pack_skip_halves(s, X, skip_w(P, prefix, b - 4));
        }
        if (st < 9) {
            const float* in_w = P.get(blk_name(prefix, st) + ".self_attn.in_proj_weight");
            for (int grp = 0; grp < 3; ++grp) pack_gemm(s, X, in_w, 384, 128, range(8 * grp, 8 * grp + 8), range(0, 8));
        } else if (back) {
            pack_out_matrix(s, X, back, 4);
        }
        if (int e = whole_stages(s, 16, "rows8")) return e;
    }
    pad_units(s, 2 * 16);
    return 0;
}

// staged streams (k_vae.hip k_vae_rows: MotionPrior decode / encode, the pose-space Denoiser steps): [stage][wave][units], every wave of a stage the same
// number of units, kVaeRing units of padding behind the last (its ring reads past its slice).  content(s, st, w) appends wave w's units of stage st.
template <class Content>
int pack_staged_stream(std::vector<uint4>& all, uint32_t* stage_base, uint32_t* stage_units, Content&& content) {
    for (int st = 0; st < kVaeStages; ++st) {
        stage_base[st] = (uint32_t)(all.size() / kUnit);
        size_t per_wave = 0;
        for (int w = 0; w < 4; ++w) {
            const size_t before = all.size();
            content(all, st, w);
            if (w == 0) per_wave = all.size() - before;
            else if (all.size() - before != per_wave) return fail(AMUSE_ESTATE, "internal: uneven wave streams in stage %d of a staged stream", st);
        }
        stage_units[st] = (uint32_t)(per_wave / kUnit);
    }
    pad_units(all, kVaeRing);
    return 0;
}
// ... and what wave w holds in stage st of a U-Net skip stack of encoder-shaped blocks (the prior's two stacks - its decoder's cross-attention is not in the
// stream - and the trans_enc pose Denoiser): st >= 1: block st - 1's out_proj k-slice, linear1 / linear2 slices of 8 hidden tiles [+ blocks 4..7: the skip
// linear's k-tiles 4w..4w+3]; st < 9: block st's q, k, v tiles of head w.  The caller puts its embedding in front of stage 0 and its output matrix behind stage 9.
void pack_skipnet_stage(std::vector<uint4>& s, int prec, const Params& P, const std::string& prefix, int st, int w) {
    if (st >= 1) {
        const int b = st - 1;
        pack_outproj_ffn(s, prec, P, blk_name(prefix, b), w);
        if (b >= 4 && b <= 7) pack_skiplin(s, prec, P, prefix, b - 4, w);
    }
    if (st < 9) pack_qkv(s, prec, P.get(blk_name(prefix, st) + ".self_attn.in_proj_weight"), w, false);
}
// the staged kernels' share of the embedding (two output tiles per wave) and of the output matrix (six per wave)
void pack_in_matrix_wave(std::vector<uint4>& s, int prec, const float* w_emb, int w) { pack_gemm(s, prec, w_emb, 128, kFeats, {2 * w, 2 * w + 1}, range(0, 22)); }
void pack_out_matrix_wave(std::vector<uint4>& s, int prec, const float* w_out, int w) { pack_gemm(s, prec, w_out, kFeats, 128, range(6 * w, 6 * w + 6), range(0, 8)); }

// 4-wave ring streams (k_sampler.hip, k_sampler_dec.hip): [wave][units of one pass over the network + kRing], the tail a copy of the head (ring wrap), every
// wave the same number of units.  content(s, w) appends wave w's pass.
template <class Content>
int pack_ring4_stream(std::vector<uint4>& all, uint32_t* wave_units, Content&& content) {
    size_t per_wave = 0;
    for (int w = 0; w < 4; ++w) {
        const size_t before = all.size();
        content(all, w);
        if (w == 0) per_wave = all.size() - before;
        else if (all.size() - before != per_wave) return fail(AMUSE_ESTATE, "internal: uneven wave streams of a 4-wave ring stream");
        all.resize(all.size() + (size_t)kRing * kUnit);
        memcpy(all.data() + before + per_wave, all.data() + before, (size_t)kRing * kUnit * sizeof(uint4));
    }
    *wave_units = (uint32_t)(per_wave / kUnit);
    return 0;
}

// 8-wave sampler streams (k_sampler8.hip on bf16 / fp16 operands, k_sampler8x.hip on split-fp16 unit pairs): wave w8 = 4 s + h; the A waves (s = 0) carry head
// h's attention weights + FFN quarters 0,1, the B waves quarters 2,3; laid out [4 A waves][units_a + kRing8 (ring wrap: tail = head)] then [4 B waves][units_b]
// (+ kRing8 units of padding behind the fp32x stream: the last B wave's initial ring fill reads past its slice).  Per block, in issue order:
//   B wave:            [ahead of an output block: the skip linear's x half (k-tiles 0..7) of output tiles 2h, 2h+1] | F1a F1b F2a F2b
//   A wave, 16-bit:    a group of 32 = 8 leading units, then q,k | v.  The leading 8 are out_proj - or, ahead of an output block, the skip-input half (k-tiles
//                      8..15 of cat(x, skip)) of the skip linear for output tiles 2h, 2h+1, with out_proj following as a group of its own | F1a F1b F2a F2b
//   A wave, fp32x:     lead (v - or, ahead of an output block, that skip-input half) | q,k for k-pairs 0,1 | [v, output blocks] | q,k for k-pairs 2,3 | out_proj
//                      | F1a F1b F2a F2b
// where F1x / F2x are linear1's output tiles / linear2's k-tiles 8h + 2q, 8h + 2q + 1 of the wave's two FFN quarters q.
int pack_sample8_streams(std::vector<uint4>& all, uint32_t* units_ab, int prec, const Params& D) {
    for (int w8 = 0; w8 < 8; ++w8) {
        const int h = w8 & 3, sgrp = w8 >> 2;
        const size_t before = all.size();
        for (int b = 0; b < 9; ++b) {
            const BlockW W = block_w(D, blk_name("encoder", b));
            const float* wskip = b >= 5 ? skip_w(D, "encoder", b - 5) : nullptr;
            const std::vector<int> out2 = {2 * h, 2 * h + 1};
            const auto outproj = [&] { pack_gemm(all, prec, W.out_w, 128, 128, range(0, 8), out2); };
            if (sgrp == 1) {
                if (wskip) pack_gemm(all, prec, wskip, 128, 256, out2, range(0, 8));
            } else if (prec != PREC_F16X2) {
                if (wskip) pack_gemm(all, prec, wskip, 128, 256, out2, range(8, 16));
                else outproj();
                pack_qkv(all, prec, W.in_w, h, true);
                if (wskip) outproj();
            } else {
                const std::vector<int> qk_tiles = {2 * h, 2 * h + 1, 8 + 2 * h, 8 + 2 * h + 1};
                const auto vproj = [&] { pack_gemm(all, prec, W.in_w, 384, 128, {16 + 2 * h, 16 + 2 * h + 1}, range(0, 8)); };
                if (wskip) pack_gemm(all, prec, wskip, 128, 256, out2, range(8, 16));
                else vproj();
                pack_gemm(all, prec, W.in_w, 384, 128, qk_tiles, range(0, 4));
                if (wskip) vproj();
                pack_gemm(all, prec, W.in_w, 384, 128, qk_tiles, range(4, 8));
                outproj();
            }
            const int qa = 8 * h + 4 * sgrp, qb = qa + 2;   // first hidden tile of the wave's two FFN quarters
            pack_f1(all, prec, W, qa, 2); pack_f1(all, prec, W, qb, 2); pack_f2(all, prec, W, qa, 2); pack_f2(all, prec, W, qb, 2);
        }
        const size_t n = all.size() - before;
        if (h == 0) units_ab[sgrp] = (uint32_t)(n / kUnit);
        else if (n / kUnit != units_ab[sgrp]) return fail(AMUSE_ESTATE, "internal: uneven 8-wave denoiser streams");
        if (sgrp == 0) {   // ring wrap: tail = head
            all.resize(all.size() + (size_t)kRing8 * kUnit);
            memcpy(all.data() + before + n, all.data() + before, (size_t)kRing8 * kUnit * sizeof(uint4));
        }
    }
    if (prec == PREC_F16X2) pad_units(all, kRing8);
    return 0;
}

}  // namespace
