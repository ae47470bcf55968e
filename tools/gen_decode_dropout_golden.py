"""tests/golden/decode_dropout.npz: the reference's own MotionPrior.decode in train() mode with the dropout masks of the library's contract
(include/amuse_hip.h, amuse_set_decode_dropout) injected - build container only (needs the reference checkout that oracle/gen_golden.py reads).

The module runs as it is; only torch.nn.functional.dropout is replaced, by a function that counts its calls (call n of a decode = layer n // 6,
site n % 6, in execution order: input blocks 0-3, middle block, output blocks 0-3), builds the contract's keep mask of that (layer, site) in
the shape of the tensor it is handed and returns where(keep, x * 1 / (1 - p), 0).  54 calls per decode are asserted.  With a replacement that
returns x unchanged the train-mode module equals the eval module bitwise (asserted below), so the replacement injects the masks and nothing else.

Usage: PYTHONDONTWRITEBYTECODE=1 python tools/gen_decode_dropout_golden.py

The fixture holds every frame of one clip per case and every 6th frame of the others (a committed file stays below 1 MiB); every frame of a clip
depends on all of the clip's masks through the self-attention, so the thinned clips pin them too."""
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.dont_write_bytecode = True

from amuse_amd import weights as wts  # noqa: E402
from oracle import gen_golden  # noqa: E402
from oracle.amuse_oracle import philox4x32_10  # noqa: E402

S, H, D, FF = 300, 4, 128, 512
P, SEED, EPOCH = 0.1, 0x9E37_79B9_7F4A_7C15, 5
CLIPS = (7, 8, 4096)
SITE_ELEMS = (H * S * S, S * D, H * S, S * D, S * FF, S * D)


def keep_mask(seed, clip, layer, site, epoch, p):
    """bool [SITE_ELEMS[site]]: element e = draw e % 4 of Philox4x32-10(key = seed, counter = (clip, 0x80000000 | (8 layer + site), e / 4, 2 + epoch));
    keep <=> draw >> 8 >= (uint32)(p 2^24)."""
    n4 = SITE_ELEMS[site] // 4
    ctr = np.zeros((n4, 4), dtype=np.uint64)
    ctr[:, 0] = np.uint64(clip & 0xFFFFFFFF)
    ctr[:, 1] = np.uint64(0x80000000 | (8 * layer + site))
    ctr[:, 2] = np.arange(n4, dtype=np.uint64)
    ctr[:, 3] = np.uint64((2 + epoch) & 0xFFFFFFFF)
    draws = philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)).reshape(-1)
    thr = int(np.float32(p) * np.float32(16777216.0))
    return (draws >> np.uint64(8)) >= np.uint64(thr)


class MaskInjector:
    """Stands in for torch.nn.functional.dropout during one MotionPrior.decode."""

    def __init__(self, clips, seed, epoch, p):
        self.clips, self.seed, self.epoch, self.p = clips, seed, epoch, p
        self.scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
        self.calls = 0

    def __call__(self, x, p=0.5, training=True, inplace=False):
        assert training and abs(p - self.p) < 1e-12, (p, training)
        layer, site = divmod(self.calls, 6)
        self.calls += 1
        B = len(self.clips)
        keep = np.stack([keep_mask(self.seed, c, layer, site, self.epoch, self.p) for c in self.clips])   # [B][elements]
        if site == 0:
            keep = keep.reshape(B * H, S, S)               # the reference's (b h) leading index
        elif site == 2:
            keep = keep.reshape(B * H, S, 1)
        else:
            keep = keep.reshape(B, S, -1).transpose(1, 0, 2)   # (B, S, F) -> the reference's (S, B, F)
        assert tuple(x.shape) == keep.shape, (layer, site, tuple(x.shape), keep.shape)
        return torch.where(torch.from_numpy(np.ascontiguousarray(keep)), x * self.scale, torch.zeros_like(x))


def main():
    import torch.nn.functional as F
    _, prior, _ = gen_golden.build_reference()
    gen_golden.load_weights(prior, wts.make_prior_weights(0))
    g = torch.Generator().manual_seed(7011)
    z = torch.randn(3, 128, generator=g)
    full, ragged = [S, S, S], [S, 217, 1]
    real = F.dropout
    with torch.no_grad():
        prior.eval()
        ev = [prior.decode(z[None], ln) for ln in (full, ragged)]
        prior.train()
        calls = [0]

        def identity(x, p=0.5, training=True, inplace=False):
            calls[0] += 1
            return x
        F.dropout = identity
        try:
            for ln, e in zip((full, ragged), ev):
                assert torch.equal(prior.decode(z[None], ln), e), "train mode with identity dropout must equal eval mode bitwise"
            assert calls[0] == 2 * 54, calls[0]
            out = []
            for ln in (full, ragged):
                inj = MaskInjector(CLIPS, SEED, EPOCH, P)
                F.dropout = inj
                out.append(prior.decode(z[None], ln).numpy())
                assert inj.calls == 54, inj.calls
        finally:
            F.dropout = real
    f_full, f_rag = out
    assert f_full.shape == (3, S, 333) and np.all(f_rag[1, 217:] == 0) and np.all(f_rag[2, 1:] == 0)
    print("dropout vs eval, max |difference|:", float(np.abs(f_full - ev[0].numpy()).max()))
    dst = REPO / "tests" / "golden" / "decode_dropout.npz"
    np.savez_compressed(dst, z=z.numpy(), lengths_ragged=np.array(ragged, dtype=np.int32), clips=np.array(CLIPS, dtype=np.uint64),
                        p=np.float32(P), seed=np.uint64(SEED), epoch=np.uint32(EPOCH), stride=np.int32(6),
                        full_clip0=f_full[0], full_thin12=f_full[1:, ::6].copy(),            # every frame of clip 0, frames 0, 6, .. of clips 1 and 2
                        ragged_clip1=f_rag[1, :217].copy(), ragged_thin02=f_rag[::2, ::6].copy())   # the 217 valid frames of clip 1, frames 0, 6, .. of clips 0 and 2
    print(dst, dst.stat().st_size, "bytes")
    assert dst.stat().st_size < (1 << 20)


if __name__ == "__main__":
    main()
