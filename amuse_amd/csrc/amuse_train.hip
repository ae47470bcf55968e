// The training step's host code: the amuse_train_* entry points (include/amuse_hip.h) over the launchers of k_train.hip, k_train_gemm.hip and k_train_attn.hip (whose
// two entry points stay beside their kernels) - the per-device state, the GEMM and weight-gradient dispatch, and the two layer sequences.  No kernel here.
//
//   per-device state   ONE table, one accessor (TrainState), one lock: the dropout epoch word; per lane the weight-gradient workspace, the generic GEMM's split-k
//                      workspace and the side stream with its fork / join events.  Everything in it is made on first use and kept for the life of the process.
//   the stream         is a parameter of everything that launches.
//   a layer pass       (LayerPass) is an object the backward sequence creates and hands to what may park a reduction in the layer's one summing launch; outside a
//                      layer those get null and add up at once.
//   fork and join      of the decoder layers' side branch are a scope guard (SideFork): whatever ends the call after the fork joins first.

#include <algorithm>
#include <mutex>

#include "amuse_host.hpp"

namespace amuse {
namespace {
#define TRY(expr) do { if (int e_ = (expr)) return e_; } while (0)

// Two chains of layers may be in flight on two streams of a device (the trainer runs the Denoiser's forward / backward pass beside the prior's): every scratch buffer
// exists once per LANE, a small integer the calling thread sets in front of its calls (amuse_train_set_lane; 0 unless told otherwise)
constexpr int kTrainLanes = 2;
constexpr int kTrainDevices = 64;
constexpr size_t kWgradWsFloats = (size_t)16 << 20;   // 64 MB of partial blocks per device and lane: every weight gradient of one layer (10.7 M floats at 9,600 rows) until the layer's summing launch
struct TrainLane {
    float* wgrad_ws;    // kWgradWsFloats: the chunk partials of the weight gradients (k_train_wgrad)
    float* splitk_ws;   // the partial tiles of k_train_gemm.hip's generic kernel
    // a stream of the library's own for the decoder layers' memory-token branch (amuse_train_layer_bwd), with the one fork / join event pair it needs; created on
    // the first (eager) call that takes the branch, so that a later graph capture of the step finds them
    hipStream_t side;
    hipEvent_t fork, join;
    bool side_ok;
};
// The dropout epoch: ONE device word per GPU that every mask-drawing kernel adds into the high half of its Philox counter's offset.  It stays 0 in eager training (the
// host hands every call a fresh offset); a training step captured as a HIP graph replays with FROZEN host offsets, so the graph ends with k_train_epoch_set and every
// replay draws fresh masks (amuse_train_epoch_advance; forward and backward of one step see the same value).  The sampling kernels' train-mode dropout (k_sampler*.hip)
// reads the same word: counter word 3 of their masks is 2 + epoch.
struct TrainDevice {
    uint32_t* epoch;
    TrainLane lane[kTrainLanes];
};
TrainDevice g_train_dev[kTrainDevices] = {};
std::mutex g_train_mu;
thread_local int g_train_lane = 0;

// The one accessor: the current device's state and the calling thread's lane of it, locked while the object lives (what the state points to never goes away: it is
// used after the lock has gone)
struct TrainState {
    std::unique_lock<std::mutex> lock;
    TrainDevice* dev = nullptr;
    TrainLane* lane = nullptr;
    int get() {
        int d = 0;
        HIP_TRY(hipGetDevice(&d));
        if (d < 0 || d >= kTrainDevices) return fail(AMUSE_EINVAL, "device %d: the training state holds devices 0 .. %d", d, kTrainDevices - 1);
        lock = std::unique_lock<std::mutex>(g_train_mu);
        dev = &g_train_dev[d];
        lane = &dev->lane[g_train_lane];
        return 0;
    }
};
int wgrad_ws(float** ws) {
    TrainState s;
    TRY(s.get());
    if (!s.lane->wgrad_ws) HIP_TRY(hipMalloc((void**)&s.lane->wgrad_ws, kWgradWsFloats * sizeof(float)));
    *ws = s.lane->wgrad_ws;
    return 0;
}
int side_stream(TrainLane** side) {
    TrainState s;
    TRY(s.get());
    if (!s.lane->side_ok) {
        HIP_TRY(hipStreamCreateWithFlags(&s.lane->side, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&s.lane->fork, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&s.lane->join, hipEventDisableTiming));
        s.lane->side_ok = true;
    }
    *side = s.lane;
    return 0;
}
}  // namespace

// Created on first use (which must not be inside a stream capture): allocated under the lock (threads of one process may race here), zeroed and the zeroing complete
// before any kernel of any stream can read it - hipMemset is ordered on the null stream only, which non-blocking streams do not wait for - and published only after
// all of that succeeded (a failed attempt leaves nothing behind and can be retried).
uint32_t* train_epoch_ptr() {
    TrainState s;
    if (s.get()) return nullptr;
    if (!s.dev->epoch) {
        uint32_t* p = nullptr;
        if (hipMalloc((void**)&p, 256) != hipSuccess) return nullptr;
        if (hipMemset(p, 0, 256) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
            (void)hipFree(p);
            return nullptr;
        }
        s.dev->epoch = p;
    }
    return s.dev->epoch;
}
hipError_t train_splitk_ws(size_t floats, float** ws) {
    TrainState s;
    if (s.get()) return hipErrorInvalidDevice;
    if (!s.lane->splitk_ws) {
        const hipError_t e = hipMalloc((void**)&s.lane->splitk_ws, floats * sizeof(float));
        if (e != hipSuccess) return e;
    }
    *ws = s.lane->splitk_ws;
    return hipSuccess;
}

namespace {
int drop_args(float p, uint32_t* thr, float* scale) {
    if (!(p >= 0.f) || p >= 1.f) return fail(AMUSE_EINVAL, "dropout probability %g outside [0, 1)", (double)p);
    *thr = (uint32_t)(p * 16777216.0f);
    *scale = 1.0f / (1.0f - p);
    return 0;
}

// The backward pass of one layer: its reductions (column sums of norms / biases, chunk sums of weight gradients) are parked in `sums` by the launches of the layer and
// added up by ONE launch at its end (launch_train_layer_sums); nothing inside the layer reads a parameter gradient.  Column-sum partials go to region nj of the
// caller's `ws`, weight-gradient partials behind one another in the lane's workspace.
struct LayerPass {
    TrainSums sums;
    size_t wgrad_used;   // floats of the weight-gradient workspace holding parked partials
    float* ws;           // amuse_train_layer::ws
    float* region() const { return ws + sums.nj * kTrainWsRegion; }
};
// the partial sums a column-sum kernel left in `ws` (n rows of ncol; outs o0 | o1 | o2 take C columns each): parked in the layer's pass, or - no pass - added up at once
int sum_columns(LayerPass* P, const float* ws, int n, float* o0, float* o1, float* o2, int ncol, int C, hipStream_t st) {
    if (!P || P->sums.nj >= 8) return launch_train_finalize(ws, n, o0, o1, o2, ncol, C, st);
    P->sums.j[P->sums.nj++] = FinJob{ws, {o0, o1, o2}, n, ncol, C};
    return 0;
}
// (in a pass the partial sums go to the pass's next region, `ws` is not looked at)
int ln_bwd(LayerPass* P, const float* dout, const float* dout2, const float* zhat, const float* rstd, const float* gamma, uint32_t thr, float scale, uint64_t seed, uint64_t off,
           long rows, float* dx, float* dy, float* dgamma, float* dbeta, float* dbias, float* ws, hipStream_t st) {
    if (P) ws = P->region();
    int n;
    TRY(launch_train_ln_bwd(dout, dout2, zhat, rstd, gamma, thr, scale, seed, off, rows, dx, dy, ws, &n, st));
    return sum_columns(P, ws, n, dgamma, dbeta, dbias, 384, 128, st);
}
int bgd_bwd(LayerPass* P, const float* da, const float* h, const float* b, uint32_t thr, float scale, uint64_t seed, uint64_t off, long rows, int F, float* dh, float* db,
            float* ws, hipStream_t st) {
    if (P) ws = P->region();
    int n;
    TRY(launch_train_bgd_bwd(da, h, b, thr, scale, seed, off, rows, F, dh, ws, &n, st));
    return sum_columns(P, ws, n, db, nullptr, nullptr, F, F, st);
}
int colsum(LayerPass* P, const float* x, long rows, int C, float* out, float* ws, hipStream_t st) {
    if (P) ws = P->region();
    int n;
    TRY(launch_train_colsum(x, rows, C, ws, &n, st));
    return sum_columns(P, ws, n, out, nullptr, nullptr, C, C, st);
}

// ---- the layer's plain GEMMs run on the library's own fp32-MFMA kernels (k_train_gemm.hip: the tall projections; the generic kernel for every other shape) and on the
// chunked weight-gradient kernel (k_train.hip k_train_wgrad): no vendor BLAS anywhere in the library.
// Weight gradients dW[M][N] = dy^T x with a long reduction: the rows are cut into chunks whose partial blocks go to the lane's workspace, behind the ones the layer's pass
// has parked, and are added up in order - by the pass's summing launch, or (no pass) right away.
long wgrad_chunks(long rows) { return std::min<long>((rows + kWgradRows - 1) / kWgradRows, kWgradMaxChunks); }
size_t wgrad_parked(long M, long N, long rows) { return wgrad_chunks(rows) > 1 ? (size_t)wgrad_chunks(rows) * M * N : 0; }   // floats a gradient leaves waiting in the workspace
// (measured, profiles/r04_train_wgrad_kernel_ab.txt: 12 us against 25 for a 128 x 128 gradient over 9,664 rows, 21 against 26 for 384 x 128; the FFN's 512 x 128 - bound by
// the fp32 MFMA rate and their 13 MB of partial blocks - 25 against 27.5 on the 64 x 32-per-wave instantiation; gradients of 131,072 elements and more go to the generic kernel)
bool wgrad_takes(long M, long N, long K) {
    return K >= 1024 && !(K & 3) && !(M & 63) && !(N & 63) && M * N < 131072L && (size_t)(M * N) * wgrad_chunks(K) <= kWgradWsFloats;
}
int wgrad(LayerPass* P, const float* dy, const float* x, float* out, long rows, long M, long N, hipStream_t st) {
    float* ws;
    TRY(wgrad_ws(&ws));
    const long chunks = wgrad_chunks(rows);
    const size_t used = P ? P->wgrad_used : 0, need = (size_t)chunks * M * N;
    if (chunks > 1 && used + need > kWgradWsFloats) return fail(AMUSE_EINVAL, "weight-gradient workspace: %zu + %zu floats of %zu", used, need, kWgradWsFloats);
    float* part = ws + used;
    TRY(launch_train_wgrad(dy, x, chunks == 1 ? out : part, rows, M, N, chunks, st));
    if (chunks == 1) return 0;
    const size_t n4 = (size_t)M * N / 4;
    if (!P || P->sums.nw >= 6) return launch_train_wgrad_sum(part, (int)chunks, n4, out, st);
    P->sums.w[P->sums.nw++] = WsumJob{part, out, (int)chunks, (unsigned)n4, P->sums.blocks};
    P->sums.blocks += (unsigned)((n4 + 255) / 256);
    P->wgrad_used += need;
    return 0;
}
// out[M][N] (+)= op(a) . op(b); a is [M][K] (ta: [K][M]), b is [K][N] (tb: [N][K]), all row-major and dense.  bias (nullable; [N]): added to every row of the product by
// the kernel's epilogue.  P: the layer pass a weight gradient parks its chunk sums in.
int rm_gemm(hipStream_t st, bool ta, bool tb, long M, long N, long K, const float* a, const float* b, float* out, bool accumulate, const float* bias = nullptr, LayerPass* P = nullptr) {
    // (the tall kernel copies 16 bytes per lane with LDS-DMA and stores pairs: operands on 16-byte, out / bias on 8-byte boundaries - the Denoiser's weights, views into the
    // trainer's flat parameter buffer behind the prior's 333-element bias, sit on 4-byte ones)
    const bool aligned = !(((uintptr_t)a | (uintptr_t)b) & 15) && !(((uintptr_t)out | (uintptr_t)bias) & 7);
    if (!ta && aligned && train_gemm_tall_takes(M, N, K, tb, bias != nullptr)) {
        HIP_TRY(launch_train_gemm_tall(a, b, bias, out, M, N, K, tb, accumulate, st));
        return 0;
    }
    if (bias && accumulate) return fail(AMUSE_EINVAL, "rm_gemm: bias and accumulate together");
    if (ta && !tb && !accumulate && !bias && wgrad_takes(M, N, K)) return wgrad(P, a, b, out, K, M, N, st);
    HIP_TRY(launch_train_gemm_any(a, b, bias, out, M, N, K, ta, tb, accumulate, st));   // every other shape: 333-wide, 32 / 160 rows, short or wide gradients
    return 0;
}
int linear_bwd(LayerPass* P, const float* dy, const float* x, const float* W, long rows, int K, int N, float* dW, float* db, float* dx, bool accumulate_dx, float* ws,
               hipStream_t st) {
    if (dW) TRY(rm_gemm(st, true, false, N, K, rows, dy, x, dW, false, nullptr, P));   // dW[N][K] = dy^T x
    if (db) TRY((N & 3) ? launch_train_colsum_any(dy, rows, N, db, ws, st) : colsum(P, dy, rows, N, db, ws, st));
    if (dx) TRY(rm_gemm(st, false, false, rows, K, N, dy, W, dx, accumulate_dx));      // dx[rows][K] (+)= dy W
    return 0;
}

// Everything a layer call can refuse is refused HERE, before its first launch: missing buffers (the self-attention's included), shapes, the dropout probabilities
// (handed back as the kernels take them: the layer's dropouts, the attention's), the epoch word, the weight-gradient workspace.
struct LayerDrop {
    uint32_t thr, thr_a;
    float scale, scale_a;
};
int layer_check(const amuse_train_layer* L, bool bwd, LayerDrop* d) {
    if (!L) return fail(AMUSE_EINVAL, "layer is NULL");
    if (L->rows < 1 || L->B < 1 || L->S < 1 || (long)L->B * L->S != L->rows) return fail(AMUSE_EINVAL, "rows %ld != B %d x S %d", L->rows, L->B, L->S);
    if (L->H < 1 || 32 % L->H) return fail(AMUSE_EINVAL, "heads %d must divide 32 (128 features, whole float4 groups per head)", L->H);
    if (L->ff < 4 || L->ff > 1024 || (L->ff & 3)) return fail(AMUSE_EINVAL, "ff %d must be a multiple of 4 up to 1024", L->ff);
    if (!L->Wo || !L->g1 || !L->be1 || !L->W1 || !L->b1 || !L->W2 || !L->g3 || !L->be3 || !L->x || !L->o2 || !L->x1 || !L->h || !L->a || !L->out || !L->tmp)
        return fail(AMUSE_EINVAL, "amuse_train_layer: a required pointer is NULL");
    if (L->mem && (!L->Wv || !L->Wc || !L->g2 || !L->be2 || !L->c || !L->vk || !L->xm)) return fail(AMUSE_EINVAL, "amuse_train_layer: decoder pointers missing");
    if (L->Win && (!L->qkv || !L->lse || L->H != 4 || L->S > 304))
        return fail(AMUSE_EINVAL, "amuse_train_layer: self-attention asked for without qkv / lse buffers, or heads != 4, or S %d > 304", L->S);
    if (bwd) {
        if (!L->dout || !L->dx || !L->do2 || !L->zh1 || !L->r1 || !L->zh3 || !L->r3 || !L->s128a || !L->s128b || !L->s512a || !L->s512b || !L->ws || !L->dWo || !L->dg1 ||
            !L->dbe1 || !L->dW1 || !L->db1 || !L->dW2 || !L->dg3 || !L->dbe3)
            return fail(AMUSE_EINVAL, "amuse_train_layer (backward): a required pointer is NULL");
        if (L->mem && (!L->zh2 || !L->r2 || !L->sdc || !L->dWv || !L->dbv || !L->dWc || !L->dg2 || !L->dbe2 || !L->dmem))
            return fail(AMUSE_EINVAL, "amuse_train_layer (backward): decoder pointers missing");
        if (L->Win && (!L->dqkv || !L->dWin)) return fail(AMUSE_EINVAL, "amuse_train_layer (backward): self-attention buffers missing");
        // every weight gradient of the layer parks its partials until the summing launch: all of them must fit the workspace together
        size_t need = 0;
        const long grads[5][2] = {{128, L->ff}, {L->ff, 128}, {L->mem ? 128 : 0, 128}, {128, 128}, {L->Win ? 384 : 0, 128}};   // dW2, dW1, dWc, dWo, dWin
        for (const auto& g : grads)
            if (g[0] && wgrad_takes(g[0], g[1], L->rows)) need += wgrad_parked(g[0], g[1], L->rows);
        if (need > kWgradWsFloats) return fail(AMUSE_EINVAL, "weight-gradient workspace: the layer's partials take %zu floats of %zu", need, kWgradWsFloats);
    }
    TRY(drop_args(L->p, &d->thr, &d->scale));
    TRY(drop_args(L->p_attn, &d->thr_a, &d->scale_a));
    if (!train_epoch_ptr()) return fail(AMUSE_EHIP, "no device word for the dropout epoch");
    return 0;
}

// The decoder layers' side branch: forked from the caller's stream `st`, joined back into it when the scope ends - by join() on the way the sequence is written, by the
// destructor on every other way out, so that no return leaves the side stream running beside a call that has ended (or a capture with an open branch).
struct SideFork {
    hipStream_t st;
    TrainLane* side = nullptr;
    explicit SideFork(hipStream_t caller) : st(caller) {}
    int fork(TrainLane* lane) {
        HIP_TRY(hipEventRecord(lane->fork, st));
        side = lane;
        HIP_TRY(hipStreamWaitEvent(lane->side, lane->fork, 0));
        return 0;
    }
    int join() {
        if (!side) return 0;
        TrainLane* lane = side;
        side = nullptr;
        const hipError_t record = hipEventRecord(lane->join, lane->side), wait = hipStreamWaitEvent(st, lane->join, 0);
        HIP_TRY(record);
        HIP_TRY(wait);
        return 0;
    }
    ~SideFork() { (void)join(); }
};
}  // namespace
}  // namespace amuse

using namespace amuse;

extern "C" {

int amuse_train_set_lane(int lane) {
    if (lane < 0 || lane >= kTrainLanes) return fail(AMUSE_EINVAL, "lane %d (0 .. %d)", lane, kTrainLanes - 1);
    g_train_lane = lane;
    return 0;
}

size_t amuse_train_ws_floats(void) { return 8 * kTrainWsRegion; }   // 8 regions of [workgroups][up to 1,024 columns]: one per reduction of a layer's backward pass

int amuse_train_ln_fwd(const float* x, const float* y, const float* bias, const float* gamma, const float* beta, float p, uint64_t seed, uint64_t offset,
                       long rows, float* out, float* zhat, float* rstd, void* stream) {
    if (!y || !gamma || !beta || !out) return fail(AMUSE_EINVAL, "amuse_train_ln_fwd: y, gamma, beta, out must be given");
    if (rows < 1) return fail(AMUSE_EINVAL, "rows must be >= 1, got %ld", rows);
    uint32_t thr; float scale;
    TRY(drop_args(p, &thr, &scale));
    return launch_train_ln_fwd(x, y, bias, gamma, beta, thr, scale, seed, offset, rows, out, zhat, rstd, (hipStream_t)stream);
}

int amuse_train_ln_bwd(const float* dout, const float* dout2, const float* zhat, const float* rstd, const float* gamma, float p, uint64_t seed, uint64_t offset, long rows,
                       float* dx, float* dy, float* dgamma, float* dbeta, float* dbias, float* ws, void* stream) {
    if (!dout || !zhat || !rstd || !gamma || !dy || !ws) return fail(AMUSE_EINVAL, "amuse_train_ln_bwd: NULL argument");
    if (rows < 1) return fail(AMUSE_EINVAL, "rows must be >= 1, got %ld", rows);
    uint32_t thr; float scale;
    TRY(drop_args(p, &thr, &scale));
    return ln_bwd(nullptr, dout, dout2, zhat, rstd, gamma, thr, scale, seed, offset, rows, dx, dy, dgamma, dbeta, dbias, ws, (hipStream_t)stream);
}

int amuse_train_bias_gelu_drop_fwd(const float* h, const float* b, float p, uint64_t seed, uint64_t offset, long rows, int F, float* out, void* stream) {
    if (!h || !b || !out) return fail(AMUSE_EINVAL, "amuse_train_bias_gelu_drop_fwd: NULL argument");
    if (rows < 1 || F < 4 || F > 1024 || (F & 3)) return fail(AMUSE_EINVAL, "rows %ld / F %d: F must be a multiple of 4 up to 1024", rows, F);
    uint32_t thr; float scale;
    TRY(drop_args(p, &thr, &scale));
    return launch_train_bgd_fwd(h, b, thr, scale, seed, offset, rows, F, out, (hipStream_t)stream);
}

int amuse_train_bias_gelu_drop_bwd(const float* da, const float* h, const float* b, float p, uint64_t seed, uint64_t offset, long rows, int F, float* dh,
                                   float* db, float* ws, void* stream) {
    if (!da || !h || !b || !dh || !db || !ws) return fail(AMUSE_EINVAL, "amuse_train_bias_gelu_drop_bwd: NULL argument");
    if (rows < 1 || F < 4 || F > 1024 || (F & 3)) return fail(AMUSE_EINVAL, "rows %ld / F %d: F must be a multiple of 4 up to 1024", rows, F);
    uint32_t thr; float scale;
    TRY(drop_args(p, &thr, &scale));
    return bgd_bwd(nullptr, da, h, b, thr, scale, seed, offset, rows, F, dh, db, ws, (hipStream_t)stream);
}

int amuse_train_colsum(const float* x, long rows, int C, float* out, float* ws, void* stream) {
    if (!x || !out || !ws) return fail(AMUSE_EINVAL, "amuse_train_colsum: NULL argument");
    if (rows < 1 || C < 4 || C > 1024 || (C & 3)) return fail(AMUSE_EINVAL, "rows %ld / C %d: C must be a multiple of 4 up to 1024", rows, C);
    return colsum(nullptr, x, rows, C, out, ws, (hipStream_t)stream);
}

int amuse_train_adamw(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, double lr, double beta1, double beta2, double eps,
                      double weight_decay, long step, void* stream) {
    if (!param || !grad || !exp_avg || !exp_avg_sq) return fail(AMUSE_EINVAL, "amuse_train_adamw: NULL argument");
    if (n < 1 || step < 1) return fail(AMUSE_EINVAL, "n %zu, step %ld (1-based)", n, step);
    // (the scalars in double on the host, as torch's Python optimizer computes them: 1 - 0.999 in fp32 is 4.7e-5 off)
    const double bc1 = 1.0 - pow(beta1, (double)step), rbc2 = 1.0 / sqrt(1.0 - pow(beta2, (double)step));
    return launch_train_adamw(param, grad, exp_avg, exp_avg_sq, n, (float)(lr / bc1), (float)(1.0 - lr * weight_decay), (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2),
                              (float)eps, (float)rbc2, (hipStream_t)stream);
}

int amuse_train_adamw_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, double lr, double beta1, double beta2, double eps,
                          double weight_decay, long* step_dev, float* scal_dev, int advance, void* stream) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || !step_dev || !scal_dev) return fail(AMUSE_EINVAL, "amuse_train_adamw_dev: NULL argument");
    if (n < 1) return fail(AMUSE_EINVAL, "n %zu", n);
    if (advance) TRY(launch_train_adamw_scalars(step_dev, lr, beta1, beta2, scal_dev, (hipStream_t)stream));
    return launch_train_adamw_dev(param, grad, exp_avg, exp_avg_sq, n, scal_dev, (float)(1.0 - lr * weight_decay), (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2),
                                  (float)eps, (hipStream_t)stream);
}

int amuse_train_epoch_advance(unsigned add, void* stream) { return launch_train_epoch_set((uint32_t)add, 0u, 0, (hipStream_t)stream); }
int amuse_train_epoch_set(unsigned value, void* stream) { return launch_train_epoch_set(0u, (uint32_t)value, 1, (hipStream_t)stream); }

// ---- layer-level entry points: everything of a transformer layer in ONE call each way (amuse_hip.h amuse_train_layer)
int amuse_train_linear_fwd(const float* x, const float* W, const float* b, long rows, int K, int N, float* out, void* stream) {
    if (!x || !W || !out) return fail(AMUSE_EINVAL, "amuse_train_linear_fwd: NULL argument");
    if (rows < 1 || K < 1 || N < 1) return fail(AMUSE_EINVAL, "rows %ld, K %d, N %d", rows, K, N);
    return rm_gemm((hipStream_t)stream, false, true, rows, N, K, x, W, out, false, b);
}

int amuse_train_linear_bwd(const float* dy, const float* x, const float* W, long rows, int K, int N, float* dW, float* db, float* dx, int accumulate_dx, float* ws,
                           void* stream) {
    if (!dy || !x || !W) return fail(AMUSE_EINVAL, "amuse_train_linear_bwd: NULL argument");
    if (rows < 1 || K < 1 || N < 1 || N > 1024) return fail(AMUSE_EINVAL, "rows %ld, K %d, N %d (up to 1024)", rows, K, N);
    if (db && !ws) return fail(AMUSE_EINVAL, "the bias gradient needs the workspace");
    return linear_bwd(nullptr, dy, x, W, rows, K, N, dW, db, dx, accumulate_dx != 0, ws, (hipStream_t)stream);
}

int amuse_train_layer_fwd(const amuse_train_layer* L, void* stream) {
    LayerDrop d;
    TRY(layer_check(L, false, &d));
    const uint32_t thr = d.thr, thr_a = d.thr_a;
    const float scale = d.scale, scale_a = d.scale_a;
    hipStream_t st = (hipStream_t)stream;
    const long rows = L->rows;
    if (L->Win) {   // the self-attention in the same call: packed in-projection, then the attention core into o2
        TRY(rm_gemm(st, false, true, rows, 384, 128, L->x, L->Win, L->qkv, false, L->bin));
        TRY(amuse_train_attn_fwd(L->qkv, L->B, L->S, L->p_attn, L->seed, L->off_self, const_cast<float*>(L->o2), L->lse, nullptr, stream));
    }
    // x1 = norm1(x + dropout1(o2 Wo^T + bo))
    TRY(rm_gemm(st, false, true, rows, 128, 128, L->o2, L->Wo, L->tmp, false));
    TRY(launch_train_ln_fwd(L->x, L->tmp, L->bo, L->g1, L->be1, thr, scale, L->seed, L->off[0], rows, L->x1, L->zh1, L->r1, st));
    const float* src = L->x1;
    if (L->mem) {   // xm = norm2(x1 + dropout2(vk Wc^T + bc)), vk = the memory token's value projection under the attention dropout
        TRY(rm_gemm(st, false, true, L->B, 128, 128, L->mem, L->Wv, L->c, false, L->bv));   // (the bias in the generic kernel's epilogue: one launch; product + bias = bias + product, the same bits as pre-filling c)
        TRY(launch_train_vk(L->c, thr_a, scale_a, L->seed, L->off[4], rows, L->S, L->H, L->vk, st));
        TRY(rm_gemm(st, false, true, rows, 128, 128, L->vk, L->Wc, L->tmp, false));
        TRY(launch_train_ln_fwd(L->x1, L->tmp, L->bc, L->g2, L->be2, thr, scale, L->seed, L->off[1], rows, L->xm, L->zh2, L->r2, st));
        src = L->xm;
    }
    // out = norm3(src + dropout3(dropout(gelu(src W1^T + b1)) W2^T + b2))
    TRY(rm_gemm(st, false, true, rows, L->ff, 128, src, L->W1, L->h, false));
    TRY(launch_train_bgd_fwd(L->h, L->b1, thr, scale, L->seed, L->off[2], rows, L->ff, L->a, st));
    TRY(rm_gemm(st, false, true, rows, 128, L->ff, L->a, L->W2, L->tmp, false));
    return launch_train_ln_fwd(src, L->tmp, L->b2, L->g3, L->be3, thr, scale, L->seed, L->off[3], rows, L->out, L->zh3, L->r3, st);
}

int amuse_train_layer_bwd(const amuse_train_layer* L, void* stream) {
    LayerDrop d;
    TRY(layer_check(L, true, &d));
    const uint32_t thr = d.thr, thr_a = d.thr_a;
    const float scale = d.scale, scale_a = d.scale_a;
    hipStream_t st = (hipStream_t)stream;
    const long rows = L->rows;
    const int ff = L->ff;
    const float* src = L->mem ? L->xm : L->x1;
    LayerPass pass{{}, 0, L->ws};
    LayerPass* P = &pass;
    SideFork branch(st);
    // FFN + last norm: s128a = d(src) through the norm, s128b = d(linear2 output)
    TRY(ln_bwd(P, L->dout, nullptr, L->zh3, L->r3, L->g3, thr, scale, L->seed, L->off[3], rows, L->s128a, L->s128b, L->dg3, L->dbe3, L->db2, nullptr, st));
    TRY(rm_gemm(st, true, false, 128, ff, rows, L->s128b, L->a, L->dW2, false, nullptr, P));
    TRY(rm_gemm(st, false, false, rows, ff, 128, L->s128b, L->W2, L->s512a, false));
    TRY(bgd_bwd(P, L->s512a, L->h, L->b1, thr, scale, L->seed, L->off[2], rows, ff, L->s512b, L->db1, nullptr, st));
    TRY(rm_gemm(st, true, false, ff, 128, rows, L->s512b, src, L->dW1, false, nullptr, P));
    TRY(rm_gemm(st, false, false, rows, 128, ff, L->s512b, L->W1, L->s128b, false));      // the FFN branch's gradient of src
    if (L->mem) {
        // cross-attention + norm2: s128a <- d(x1), s128b <- d(out_proj output)
        TRY(ln_bwd(P, L->s128a, L->s128b, L->zh2, L->r2, L->g2, thr, scale, L->seed, L->off[1], rows, L->s128a, L->s128b, L->dg2, L->dbe2, L->dbc, nullptr, st));
        TRY(rm_gemm(st, true, false, 128, 128, rows, L->s128b, L->vk, L->dWc, false, nullptr, P));
        // (The same fork in the FORWARD pass - vk produced on the side stream under the self-attention half - measured 10 % SLOWER: a cross-queue edge of a replayed graph
        // takes on the order of 100 us to propagate, harmless here where the join has a whole layer of slack, fatal there where it has 40 us.)
        // The memory token's branch - d(c) per clip, dWv, dbv, d(mem): four launches over 32 rows, 5-13 us each of mostly latency - feeds nothing inside the layer.  In
        // the tall layers it runs on a stream of the library's own beside the rest of the layer (forked here, joined in front of the layer's summing launch); d(vk) then
        // sits in the forward pass's scratch `tmp`, because `do2` is written again further down.  (The side stream is made by the first call that forks, still in
        // front of the fork; the calls a captured step is made of find it made.)
        TrainLane* side = nullptr;
        if (rows >= 1024) TRY(side_stream(&side));
        float* dvk = side ? L->tmp : L->do2;
        TRY(rm_gemm(st, false, false, rows, 128, 128, L->s128b, L->Wc, dvk, false));     // d(vk)
        hipStream_t ms = st;
        if (side) {
            TRY(branch.fork(side));
            ms = side->side;
        }
        TRY(launch_train_dc(dvk, thr_a, scale_a, L->seed, L->off[4], L->B, L->S, L->H, L->sdc, ms));
        if (side) HIP_TRY(launch_train_gemm_any(L->sdc, L->mem, nullptr, L->dWv, 128, 128, L->B, true, false, false, ms));
        else TRY(rm_gemm(st, true, false, 128, 128, L->B, L->sdc, L->mem, L->dWv, false));
        TRY(colsum(P, L->sdc, L->B, 128, L->dbv, nullptr, ms));
        if (side) HIP_TRY(launch_train_gemm_any(L->sdc, L->Wv, nullptr, L->dmem, L->B, 128, 128, false, false, false, ms));
        else TRY(rm_gemm(st, false, false, L->B, 128, 128, L->sdc, L->Wv, L->dmem, false));
        TRY(ln_bwd(P, L->s128a, nullptr, L->zh1, L->r1, L->g1, thr, scale, L->seed, L->off[0], rows, L->dx, L->s128b, L->dg1, L->dbe1, L->dbo, nullptr, st));
    } else {
        TRY(ln_bwd(P, L->s128a, L->s128b, L->zh1, L->r1, L->g1, thr, scale, L->seed, L->off[0], rows, L->dx, L->s128b, L->dg1, L->dbe1, L->dbo, nullptr, st));
    }
    // self-attention's out_proj
    TRY(rm_gemm(st, true, false, 128, 128, rows, L->s128b, L->o2, L->dWo, false, nullptr, P));
    TRY(rm_gemm(st, false, false, rows, 128, 128, L->s128b, L->Wo, L->do2, false));
    if (L->Win) {   // the attention's backward pass and the in-projection's in the same call
        TRY(amuse_train_attn_bwd(L->qkv, L->o2, L->lse, L->do2, L->B, L->S, L->p_attn, L->seed, L->off_self, L->dqkv, stream));
        TRY(linear_bwd(P, L->dqkv, L->x, L->Win, rows, 128, 384, L->dWin, L->dbin, L->dx, true, nullptr, st));
    }
    TRY(branch.join());   // the summing launch reads the branch's column sums, the caller d(mem)
    return launch_train_layer_sums(pass.sums, st);   // every column sum and weight gradient of the layer
}

}  // extern "C"
