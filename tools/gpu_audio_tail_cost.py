"""Cost of the audio model's tail (include/amuse_hip.h "Audio model metrics"), in one GPU process, HIP events around synchronised work, every shape warmed up
first, N >= 20 timed calls per cell, the candidates of a cell ALTERNATING call by call and each on buffers of its own (the 268 MB weight stream is near the
Infinity Cache's size: a candidate timed back to back with itself would find part of its stream there).
  python tools/gpu_audio_tail_cost.py [--calls 20] [--out profiles/audio_tail_cost.txt]
Cells:
  1. the last Linear (131072 x 1024) at B = 1, 8, 32 in bf16: the skinny kernel (amuse_debug_tail_gemm) against the route the library had for the same product -
     k_gemm_tm through amuse_debug_gemm, epilogue 3, operands tiled / packed outside the timed region - and each as a fraction of the byte floor
     (weight bytes / 6.05 TB/s, the measured sweep rate; recorded, no bar);
  2. the same in AMUSE_PREC_F32X (537 MB of hi | lo units) beside bf16;
  3. AudioEngine.metrics per clip against two AudioEngine.features calls (the two encoder passes it contains)."""
import argparse
import ctypes as C
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from amuse_amd import _lib  # noqa: E402
from amuse_amd import audio_weights as aw  # noqa: E402
from amuse_amd.audio import AudioEngine  # noqa: E402

N, K = 1024 * 128, 1024
SWEEP = 6.05e12   # B/s
p = lambda t: C.c_void_p(t.data_ptr())


def pack_tail(w16):
    """[N, K] 16-bit -> amuse_debug_tail_pack's order: [feature tile][k-step][lane = (g, i)][e], feature = 16 tile + i, k = 32 ks + 8 g + e"""
    n, k = w16.shape
    return w16.view(n // 16, 16, k // 32, 4, 8).permute(0, 2, 3, 1, 4).contiguous()


def pack_tm(w16):
    """[N, K] bf16 -> k_gemm_tm's fragment order (amuse_audio_api.hip pack_w; tools/gpu_gemm_bench.py)"""
    n, k = w16.shape
    return w16.view(n // 64, 2, 4, 2, 4, k // 32, 4, 8).permute(0, 1, 3, 5, 6, 2, 4, 7).contiguous().view(-1)


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3   # us


def alternate(cands, calls):
    for fn in cands.values():
        for _ in range(3):
            fn()
    ts = {k: [] for k in cands}
    for _ in range(calls):
        for k, fn in cands.items():
            ts[k].append(timed(fn))
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = _lib.load()
    g = torch.Generator(device="cuda").manual_seed(0)
    lines = [f"the last Linear of AST_EVP's decoder, 131072 x 1024, {args.calls} timed calls per cell, candidates alternating call by call on buffers of their own; "
             f"us per call (median, min); floor = weight bytes / 6.05 TB/s"]
    w = torch.randn(N, K, device="cuda", generator=g) / 32.0
    bias = torch.randn(N, device="cuda", generator=g)
    wb = w.bfloat16()
    w_skinny = pack_tail(wb)
    w_tm = pack_tm(wb)
    hi = w.half()
    lo = (w - hi.float()).half()
    w_x = torch.stack((pack_tail(hi), pack_tail(lo)), dim=2).contiguous()   # [tile][ks][plane][lane][e]
    del w, hi, lo
    floor_b, floor_x = N * K * 2 / SWEEP * 1e6, N * K * 4 / SWEEP * 1e6
    out_tm = torch.empty(128, N, device="cuda", dtype=torch.float32)        # k_gemm_tm pads the rows to its 128-token tile
    for B in (1, 8, 32):
        a = torch.randn(B, K, device="cuda", generator=g)
        a_tm = torch.empty(128, K, device="cuda", dtype=torch.bfloat16)
        _lib.check(lib.amuse_debug_tile(p(a.bfloat16().contiguous()), p(a_tm), B, K, 0, None))
        out_s, out_x = torch.empty(B, N, device="cuda"), torch.empty(B, N, device="cuda")
        cands = {
            "skinny bf16": lambda: _lib.check(lib.amuse_debug_tail_gemm(p(a), p(w_skinny), p(bias), B, N, K, _lib.PREC_BF16, p(out_s), None)),
            "k_gemm_tm bf16": lambda: _lib.check(lib.amuse_debug_gemm(p(a_tm), p(w_tm), p(bias), B, N, K, 3, p(out_tm), None)),
            "skinny fp32x": lambda: _lib.check(lib.amuse_debug_tail_gemm(p(a), p(w_x), p(bias), B, N, K, _lib.PREC_F32X, p(out_x), None)),
        }
        ts = alternate(cands, args.calls)
        # the two routes compute the same product from the same bf16 operands
        back = torch.empty(B, N, device="cuda")
        _lib.check(lib.amuse_debug_tile(p(out_tm), p(back), B, N, 2, None))
        torch.cuda.synchronize()
        agree = float((back - out_s).abs().max() / out_s.abs().max())
        for k, floor in (("skinny bf16", floor_b), ("k_gemm_tm bf16", floor_b), ("skinny fp32x", floor_x)):
            med, mn = statistics.median(ts[k]), min(ts[k])
            lines.append(f"B {B:2d}  {k:15s} median {med:8.1f} us  min {mn:8.1f} us  floor {floor:5.1f} us = {floor / med:.2f} of the median")
        lines.append(f"B {B:2d}  skinny / k_gemm_tm = {statistics.median(ts['skinny bf16']) / statistics.median(ts['k_gemm_tm bf16']):.2f} x   "
                     f"fp32x / bf16 = {statistics.median(ts['skinny fp32x']) / statistics.median(ts['skinny bf16']):.2f} x   (routes agree to {agree:.1e} of max)")
    del w_skinny, w_tm, w_x, out_tm
    torch.cuda.empty_cache()

    lines.append("")
    lines.append(f"AudioEngine.metrics (one clip: 3 encoders + heads, fusion + decoder, 3 encoders again) against two AudioEngine.features calls, bf16, {args.calls} calls each, alternating; ms")
    eng = AudioEngine(*[aw.make_ast_weights(0, n) for n in aw.ENCODERS], "cuda:0", tail_sd=aw.make_ast_tail_weights(0))
    wave = (0.1 * torch.randn(1, 159744, device="cuda", generator=g))
    fb = eng.fbank(wave)
    con, emo, sty = eng.features(wave)
    cands = {"metrics": lambda: eng.metrics(fb), "2 x features": lambda: (eng.features(wave), eng.features(wave)),
             "reconstruct": lambda: eng.reconstruct(con, emo, sty, group=1)}
    ts = alternate(cands, args.calls)
    for k in cands:
        lines.append(f"{k:13s} median {statistics.median(ts[k]) / 1e3:8.3f} ms  min {min(ts[k]) / 1e3:8.3f} ms")
    lines.append(f"metrics / (2 x features) = {statistics.median(ts['metrics']) / statistics.median(ts['2 x features']):.2f} x")
    eng.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
