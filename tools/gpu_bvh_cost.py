"""Cost of BVH export on the GPU (amuse_amd/bvh.py, csrc/k_bvh.hip) -> profiles/bvh_cost.txt.  HIP events around whole calls of the entry point on preallocated
outputs (no allocation inside the timed window), after a warm-up; host steps by time.perf_counter around synchronised work.
  256 clips x 300 frames (a batch of 10 s clips: 8 launches of 32 sequences), order ZYX, scale 100:
    amuse_bvh_motion, text alone - principal values, and with unwrap (the sequential walk)
    the device-to-host copy of the 154.8 MB of text into pinned and into pageable memory
    the 256 file writes (header ++ block through a .part file and os.replace, into a temporary directory)
    the thing it replaces: the same 256 files from the same Euler values by numpy / Python '%'-formatting (one "%11.6f" per number, joined), 16 clips timed
    and scaled to 256
Nobody set a target for these: they are recorded.
usage: python tools/gpu_bvh_cost.py [out file]"""
import ctypes as C
import io
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
from amuse_amd import _lib, bvh  # noqa: E402

DEV = "cuda:0"
HBM = 8.0e12   # MI355X HBM3E peak, bytes / s (data sheet)
PARENTS = [-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 15, 15, 15,
           20, 25, 26, 20, 28, 29, 20, 31, 32, 20, 34, 35, 20, 37, 38, 21, 40, 41, 21, 43, 44, 21, 46, 47, 21, 49, 50, 21, 52, 53]


def timed(fn, n):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return np.array([a.elapsed_time(b) for a, b in ev])


def fmt(a):
    a = np.asarray(a)
    return f"{np.median(a):9.3f} ({a.min():.3f}) ms"


def main():
    out = Path(sys.argv[1]) if len(sys.argv) > 1 else REPO / "profiles" / "bvh_cost.txt"
    lib = _lib.load()
    S, F = 256, 300
    rows = S * F
    g = torch.Generator().manual_seed(0)
    poses = ((0.02 * torch.randn(S, F, 55, 3, generator=g)).cumsum(1) + 0.5 * torch.randn(S, 1, 55, 3, generator=g)).reshape(rows, 55, 3).to(DEV)
    trans = (0.01 * torch.randn(S, F, 3, generator=g)).cumsum(1).reshape(rows, 3).to(DEV)
    rr = (0.1 * torch.randn(S, 3, generator=g)).to(DEV)
    dfs = bvh.layout(PARENTS)
    text = torch.empty(rows * bvh.ROW_BYTES, dtype=torch.uint8, device=DEV)
    status = torch.zeros(S, dtype=torch.int32, device=DEV)
    fr, dd = (C.c_int * S)(*([F] * S)), (C.c_int * 55)(*[int(j) for j in dfs])
    st = torch.cuda.current_stream().cuda_stream
    vp = lambda x: C.c_void_p(x.data_ptr())

    def call(unwrap):
        _lib.check(lib.amuse_bvh_motion(vp(poses), vp(trans), vp(rr), S, fr, dd, 5, C.c_float(100.0), unwrap, None, vp(text), vp(status), st))

    lines = [f"tools/gpu_bvh_cost.py on {torch.cuda.get_device_name(0)}: {S} clips x {F} frames, order ZYX, scale 100; HIP events around whole calls, ms median (min), "
             f"100 repetitions after 5 warm-up calls; host steps by perf_counter"]
    nbytes = rows * bvh.ROW_BYTES
    for unwrap in (0, 1):
        for _ in range(5):
            call(unwrap)
        torch.cuda.synchronize()
        ts = timed(lambda: call(unwrap), 100)
        need = rows * 168 * 4 + nbytes
        lines.append(f"amuse_bvh_motion, text alone, unwrap {unwrap}: {fmt(ts)} per call ({-(-S // 32) * (1 + unwrap)} launches); it reads {rows * 168 * 4 / 1e6:.1f} MB and writes "
                     f"{nbytes / 1e6:.1f} MB of text = {need / HBM * 1e3:.4f} ms at the HBM peak; {np.median(ts) * 1e6 / (rows * 168):.3f} ns per number")
    assert not status.cpu().numpy().any()
    call(0)
    torch.cuda.synchronize()
    pinned = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
    for name, dst in (("pinned", pinned), ("pageable", torch.empty(nbytes, dtype=torch.uint8))):
        ts = []
        for _ in range(6):
            t0 = time.perf_counter()
            dst.copy_(text)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        lines.append(f"device-to-host copy of the text, {nbytes / 1e6:.1f} MB, into {name} memory: {fmt(ts[1:])} ({nbytes / np.median(ts[1:]) / 1e6:.1f} GB/s)")
    host = pinned.numpy()
    J = np.random.default_rng(0).standard_normal((55, 3)) * 0.2
    header = bvh.header_text(PARENTS, J, F, 30.0, "ZYX", 100.0)
    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        for s in range(S):
            bvh.write_bvh(Path(d) / f"clip_{s:03d}_motion.bvh", header, host[s * F * bvh.ROW_BYTES:(s + 1) * F * bvh.ROW_BYTES].tobytes())
        t_write = (time.perf_counter() - t0) * 1e3
        lines.append(f"{S} file writes (header {len(header)} B ++ block {F * bvh.ROW_BYTES} B each, .part and os.replace, a temporary directory): {t_write:9.1f} ms")
        # the thing it replaces: the same values formatted on the host
        euler = torch.empty(rows, 168, dtype=torch.float32, device=DEV)
        _lib.check(lib.amuse_bvh_motion(vp(poses), vp(trans), vp(rr), S, fr, dd, 5, C.c_float(100.0), 0, vp(euler), None, vp(status), st))
        vals = euler.cpu().numpy()
        n_host = 16
        t0 = time.perf_counter()
        for s in range(n_host):
            block = "".join(" ".join(["%11.6f"] * 168) % tuple(row) + "\n" for row in vals[s * F:(s + 1) * F].tolist()).encode("ascii")
            bvh.write_bvh(Path(d) / f"host_{s:03d}_motion.bvh", header, block)
        t_host = (time.perf_counter() - t0) * 1e3 / n_host
        assert block == host[(n_host - 1) * F * bvh.ROW_BYTES:n_host * F * bvh.ROW_BYTES].tobytes()          # the same bytes
        t0 = time.perf_counter()
        for s in range(n_host):
            buf = io.BytesIO()
            np.savetxt(buf, vals[s * F:(s + 1) * F], fmt="%11.6f", delimiter=" ")
        t_np = (time.perf_counter() - t0) * 1e3 / n_host
    lines.append(f"host formatting instead, Python '%' on a whole row at a time, written the same way: {t_host:9.2f} ms per clip ({n_host} clips timed) = {t_host * S:9.1f} ms for {S} "
                 f"(the Euler values already on the host; numpy.savetxt of the same block: {t_np:.2f} ms per clip)")
    return lines, out


if __name__ == "__main__":
    lines, out = main()
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
    print("\n".join(lines))
