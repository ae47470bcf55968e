"""The training step's fused transformer layers (amuse_amd/train_ops.py on csrc/amuse_train.hip, k_train.hip, k_train_attn.hip) restated for the tests: the dropout
masks the kernels draw, in numpy integer arithmetic, and the layers themselves in torch float64 on the CPU with those masks injected - autograd supplies the backward
pass.  tests/test_train_layer_ref_cpu.py holds this file to the eager layers of nn_modules.py and shows that the GPU bars can tell a wrong mask from rounding;
tests/test_gpu_train_layer_dropout.py holds the kernels to it.  (Not a test module.)

The mask contract, restated here on its own.  A layer call has six dropout sites, each with a call offset of its own (amuse_train_layer_fwd; train_ops._layer_forward_on
draws off[0..4] and then off_self from next_offset(), the seed is torch.initial_seed() & 0x7FFF...F):

    site     what is dropped                                         offset    element index e                        kernel
    self     self-attention probabilities (after the softmax)        off_self  hash of (b 4 + h, query i, key j)      k_attn_fwd / k_attn_bwd
    drop1    dropout1 on the self-attention out_proj + bias          off[0]    row 128 + f                            k_train_ln_fwd / _bwd
    cross    the one-key cross-attention's probability (exactly 1)   off[4]    (b S + s) H + h                        k_train_vk / k_train_dc
    drop2    dropout2 on the cross-attention out_proj + bias         off[1]    row 128 + f                            k_train_ln_fwd / _bwd
    ffn      dropout(gelu(linear1))                                  off[2]    row 512 + f                            k_train_bgd_fwd / _bwd
    drop3    the last residual branch's dropout on linear2 + bias    off[3]    row 128 + f                            k_train_ln_fwd / _bwd
             (DecoderLayer.dropout3, EncoderLayer.dropout2)

An encoder layer has the sites self, drop1, ffn and drop3 (its offsets off[1] and off[4] are drawn and not used).

Philox sites (k_train.hip drop_scale4 / head_keep): element e is draw e % 4 of Philox4x32-10 with key (seed lo, seed hi) and counter (e / 4 lo, e / 4 hi, offset lo,
offset hi), where offset += epoch << 32 (the device's dropout epoch word); kept <=> (draw >> 8) >= (uint32)(float32(p) 2^24); kept values times 1 / (1 - p) in fp32.

Self-attention (k_train_attn.hip): k = seed 0x9E3779B97F4A7C15 + offset 0xD1B54A32D192ED03 (mod 2^64); k ^= k >> 29; key = (uint32)(k ^ (k >> 32)); at an epoch other than
0, key ^= lowbias32(epoch 0x9E3779B9 + 0x85EBCA6B); idx = ((b 4 + h) 512 + i) 512 + j (mod 2^32); kept <=> lowbias32(idx ^ key) >= (uint32)(double(float32(p)) 2^32)."""
import math

import numpy as np
import torch

D, H, DH, FF = 128, 4, 32, 512
SITES = ("self", "drop1", "cross", "drop2", "ffn", "drop3")
ENC_SITES = ("self", "drop1", "ffn", "drop3")
_M32, _M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF

# the bars the GPU tests hold the fused layers to (tests/test_gpu_train_ops.py test_fused_layer_equals_the_eager_layer_in_eval_mode)
OUT_BAR, GRAD_BAR = 2e-5, 2e-4


# ---------------------------------------------------------------------------------------------------- masks
def fp32_scale(p):
    p32 = np.float32(p)
    return float(np.float32(1.0) / (np.float32(1.0) - p32))


def philox_thr(p):
    return int(np.float32(p) * np.float32(16777216.0))


def philox_keep(seed, offset, epoch, n, p):
    """bool (n,): the keep flags of elements 0 .. n - 1 of one call of a Philox site."""
    from oracle import amuse_oracle as orc
    if philox_thr(p) == 0:
        return np.ones(n, dtype=bool)
    off = (int(offset) + (int(epoch) << 32)) & _M64
    n4 = (n + 3) // 4
    e4 = np.arange(n4, dtype=np.uint64)
    ctr = np.empty((n4, 4), dtype=np.uint64)
    ctr[:, 0] = e4 & np.uint64(_M32)
    ctr[:, 1] = e4 >> np.uint64(32)
    ctr[:, 2] = np.uint64(off & _M32)
    ctr[:, 3] = np.uint64(off >> 32)
    draws = orc.philox4x32_10(ctr, (seed & _M32, (seed >> 32) & _M32)).reshape(-1)[:n]
    return (draws >> np.uint64(8)) >= np.uint64(philox_thr(p))


def row_keep(seed, offset, epoch, rows, F, p):
    """(rows, F): ln_fwd / ln_bwd (F = 128), bias_gelu_drop_fwd / _bwd (any F)"""
    return philox_keep(seed, offset, epoch, rows * F, p).reshape(rows, F)


def head_keep(seed, offset, epoch, B, S, nheads, p):
    """(B, S, nheads): the one-key cross-attention"""
    return philox_keep(seed, offset, epoch, B * S * nheads, p).reshape(B, S, nheads)


def lowbias32(x):
    """numpy uint64 holding uint32 values"""
    m = np.uint64(_M32)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & m
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & m
    return x ^ (x >> np.uint64(16))


def attn_key(seed, offset, epoch):
    k = (int(seed) * 0x9E3779B97F4A7C15 + int(offset) * 0xD1B54A32D192ED03) & _M64
    k ^= k >> 29
    key = (k ^ (k >> 32)) & _M32
    if epoch & _M32:
        key ^= int(lowbias32(np.uint64(((epoch & _M32) * 0x9E3779B9 + 0x85EBCA6B) & _M32)))
    return key


def attn_thr(p):
    return int(float(np.float32(p)) * 4294967296.0) if p > 0 else 0


def attn_keep(seed, offset, epoch, B, S, p):
    """(B, 4, S, S) [clip][head][query][key]"""
    bh = np.arange(B * 4, dtype=np.uint64)[:, None, None]
    i = np.arange(S, dtype=np.uint64)[None, :, None]
    j = np.arange(S, dtype=np.uint64)[None, None, :]
    idx = (((bh * np.uint64(512) + i) * np.uint64(512)) + j) & np.uint64(_M32)
    return (lowbias32(idx ^ np.uint64(attn_key(seed, offset, epoch))) >= np.uint64(attn_thr(p))).reshape(B, 4, S, S)


def layer_offsets(before):
    """site -> offset of a layer call made when train_ops._OFFSET[0] == before"""
    off = [before + 1 + i for i in range(5)]
    return {"drop1": off[0], "drop2": off[1], "ffn": off[2], "drop3": off[3], "cross": off[4], "self": before + 6}


class Masks:
    """mask(site, B, S) -> bool tensor of the site's shape; scale(site).  `offsets`: site -> offset (layer_offsets)."""

    def __init__(self, seed, offsets, epoch=0, p=0.1, p_attn=0.1, ff=FF):
        self.seed, self.offsets, self.epoch, self.p, self.p_attn, self.ff = seed, dict(offsets), epoch, p, p_attn, ff

    def scale(self, site):
        return fp32_scale(self.p_attn if site in ("self", "cross") else self.p)

    def __call__(self, site, B, S):
        off = self.offsets[site]
        if site == "self":
            m = attn_keep(self.seed, off, self.epoch, B, S, self.p_attn)
        elif site == "cross":
            m = head_keep(self.seed, off, self.epoch, B, S, H, self.p_attn)
        else:
            F = self.ff if site == "ffn" else D
            m = row_keep(self.seed, off, self.epoch, B * S, F, self.p).reshape(B, S, F)
        return torch.from_numpy(m)

    def with_offset(self, site, offset):
        return Masks(self.seed, dict(self.offsets, **{site: offset}), self.epoch, self.p, self.p_attn, self.ff)


class AllKeep:
    def scale(self, site):
        return 1.0

    def __call__(self, site, B, S):
        return None


def _drop(t, keep, scale):
    return t if keep is None else torch.where(keep, t * scale, torch.zeros_like(t))


# ---------------------------------------------------------------------------------------------------- layers
def _ln(z, g, b):
    mu = z.mean(-1, keepdim=True)
    d = z - mu
    return d * torch.rsqrt((d * d).mean(-1, keepdim=True) + 1e-5) * g + b


def _gelu(u):
    return 0.5 * u * (1.0 + torch.erf(u * (1.0 / math.sqrt(2.0))))


def layer_ref(kind, state_dict, x, mem, dout, masks, dtype=torch.float64):
    """nn_modules.EncoderLayer (kind "enc") / DecoderLayer ("dec", a memory of one token) written out, with a keep mask at every dropout site, in `dtype` on the CPU.
    -> {"out", "dx", "dmem" (None for "enc"), "grads": {parameter name: gradient}}; the q / k rows of the cross-attention's in-projection are zero, as autograd leaves them."""
    W = {n: t.detach().to("cpu", dtype).clone().requires_grad_(True) for n, t in state_dict.items()}
    x = x.detach().to("cpu", dtype).clone().requires_grad_(True)
    dec = kind == "dec"
    if dec:
        mem = mem.detach().to("cpu", dtype).clone().requires_grad_(True)
    B, S, E = x.shape
    # self-attention (nn_modules.mha_self): packed in-projection, heads = contiguous E / H slices, dropout on the normalised probabilities
    q, k, v = ((x @ W["self_attn.in_proj_weight"].T + W["self_attn.in_proj_bias"]).view(B, S, 3, H, DH).unbind(2))
    q, k, v = q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)                       # (B, H, S, dh)
    prob = _drop(torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(DH), dim=-1), masks("self", B, S), masks.scale("self"))
    o = (prob @ v).transpose(1, 2).reshape(B, S, E)
    y = _drop(o @ W["self_attn.out_proj.weight"].T + W["self_attn.out_proj.bias"], masks("drop1", B, S), masks.scale("drop1"))
    t = _ln(x + y, W["norm1.weight"], W["norm1.bias"])
    if dec:
        # cross-attention onto the one memory token (nn_modules.mha_one_key): the probability is 1, dropped per (clip, query, head)
        vz = mem @ W["multihead_attn.in_proj_weight"][2 * E:].T + W["multihead_attn.in_proj_bias"][2 * E:]      # (B, 1, E)
        keep = _drop(torch.ones(B, S, H, dtype=dtype), masks("cross", B, S), masks.scale("cross"))
        heads = (keep[..., None] * vz.view(B, 1, H, DH)).reshape(B, S, E)
        y = _drop(heads @ W["multihead_attn.out_proj.weight"].T + W["multihead_attn.out_proj.bias"], masks("drop2", B, S), masks.scale("drop2"))
        t = _ln(t + y, W["norm2.weight"], W["norm2.bias"])
    a = _drop(_gelu(t @ W["linear1.weight"].T + W["linear1.bias"]), masks("ffn", B, S), masks.scale("ffn"))
    y = _drop(a @ W["linear2.weight"].T + W["linear2.bias"], masks("drop3", B, S), masks.scale("drop3"))
    last = "norm3" if dec else "norm2"
    out = _ln(t + y, W[last + ".weight"], W[last + ".bias"])
    out.backward(dout.detach().to("cpu", dtype))
    return {"out": out.detach(), "dx": x.grad, "dmem": mem.grad if dec else None, "grads": {n: w.grad for n, w in W.items()}}


def tensors(res):
    """{name: tensor} of everything a layer result holds: out, dx, dmem and every parameter gradient"""
    t = {"out": res["out"], "dx": res["dx"]}
    if res["dmem"] is not None:
        t["dmem"] = res["dmem"]
    t.update(res["grads"])
    return t


def distances(got, ref):
    """{name: distance in units of its bar's scale}: |out - ref| absolute, every gradient relative to the largest entry of its reference"""
    g, r = tensors(got), tensors(ref)
    assert set(g) == set(r), (sorted(g), sorted(r))
    d = {}
    for n in r:
        a, b = g[n].detach().to("cpu", torch.float64), r[n].to(torch.float64)
        assert a.shape == b.shape, n
        err = float((a - b).abs().max())
        d[n] = err if n == "out" else err / max(float(b.abs().max()), 1e-300)
    return d


# ---------------------------------------------------------------------------------------------------- raw kernels
def ln_drop_ref(x, y, bias, gamma, beta, keep, scale, douts):
    """LayerNorm(x + dropout(y + bias)) and its backward pass for the gradient sum(douts), in float64 on the tensors' device (plain torch under autograd)
    -> out, dx, dy, dgamma, dbeta, dbias"""
    xr, yr, bi, ga, be = (t.detach().double().clone().requires_grad_(True) for t in (x, y, bias, gamma, beta))
    out = _ln(xr + _drop(yr + bi, keep, scale), ga, be)
    out.backward(sum(d.double() for d in douts))
    return out.detach(), xr.grad, yr.grad, ga.grad, be.grad, bi.grad


def gelu_drop_ref(h, b, keep, scale, da):
    """dropout(gelu(h + b)) and its backward pass in float64 -> a, dh, db"""
    hr, br = h.detach().double().clone().requires_grad_(True), b.detach().double().clone().requires_grad_(True)
    a = _drop(_gelu(hr + br), keep, scale)
    a.backward(da.double())
    return a.detach(), hr.grad, br.grad


def attn_ref(qkv, dout, B, S, keep, scale, dtype=torch.float64):
    """softmax(q k^T / sqrt(32)) . keep . scale times v for qkv (B S, 384) -> o (B S, 128), lse (B, 4, S) in log2 units with the scale folded (what k_attn_fwd
    stores), d(qkv)"""
    x = qkv.detach().to("cpu", dtype).clone().requires_grad_(True)
    q, k, v = (t.transpose(1, 2) for t in x.view(B, S, 3, H, DH).unbind(2))                  # (B, 4, S, 32)
    s = q @ k.transpose(-1, -2) / math.sqrt(DH)
    lse = torch.logsumexp(s, -1) / math.log(2.0)
    o = (_drop(torch.softmax(s, -1), keep, scale) @ v).transpose(1, 2).reshape(B * S, D)
    o.backward(dout.detach().to("cpu", dtype))
    return o.detach(), lse.detach(), x.grad


PEAKED_B, PEAKED_S, PEAKED_RAMP = 2, 300, 8.0


def peaked_case():
    """qkv (600, 384), dout (600, 128) in float32: q times 4 (scores of standard deviation 4) and a score ramp of PEAKED_RAMP over the key index - ascending on head 0,
    where the online softmax's running maximum keeps moving from key tile to key tile, descending on head 1, where it all but stands still.  (The ramp: feature 0 of every
    query of the two heads is 4, feature 0 of key j is ramp(j) sqrt(32) / 4.)"""
    B, S = PEAKED_B, PEAKED_S
    g = torch.Generator().manual_seed(77)
    qkv = torch.randn(B, S, 3, H, DH, generator=g)
    dout = torch.randn(B * S, D, generator=g)
    qkv[:, :, 0] *= 4
    ramp = torch.arange(S, dtype=torch.float32) / (S - 1) * (PEAKED_RAMP * math.sqrt(DH) / 4)
    qkv[:, :, 0, 0, 0] = 4
    qkv[:, :, 0, 1, 0] = 4
    qkv[:, :, 1, 0, 0] = ramp[None]
    qkv[:, :, 1, 1, 0] = ramp.flip(0)[None]
    return qkv.reshape(B * S, 3 * D), dout


# ---------------------------------------------------------------------------------------------------- the cases both test files use
LAYER_P = 0.1
LAYER_SEED = 0x1_2345_6789                  # torch.manual_seed(LAYER_SEED): the high word of the Philox key is not 0
LAYER_OFFSET = 4000                         # train_ops._OFFSET[0] in front of the layer call
# (kind, B, S, epoch): a ragged attention tile | one key | the decoder's memory branch on the main stream | 1,200 rows: the side-stream fork with d(vk) in tmp, the chunked
# weight-gradient kernel, two attention parts | one decoder case again at epoch 5
LAYER_CASES = [("enc", 2, 17, 0), ("enc", 1, 1, 0), ("dec", 2, 17, 0), ("dec", 4, 300, 0), ("dec", 2, 17, 5)]


def make_layer(kind, seed):
    """tests/test_gpu_train_ops.py _layers on the CPU: the module at p = 0.1 with non-trivial LayerNorm parameters and biases"""
    from amuse_amd import nn_modules as nm
    torch.manual_seed(seed)
    m = (nm.EncoderLayer if kind == "enc" else nm.DecoderLayer)(p=LAYER_P)
    for p in m.parameters():
        if p.dim() == 1:
            p.data.normal_(1.0 if p.data.mean() > 0.5 else 0.0, 0.2)
    return m


def layer_case(kind, B, S):
    """(module on the CPU, x, mem, dout) in float32"""
    m = make_layer(kind, 1)
    g = torch.Generator().manual_seed(1000 * B + S)
    x, mem, dout = (torch.randn(B, n, D, generator=g) for n in (S, 1, S))
    return m, x, mem, dout


def layer_masks(epoch=0):
    return Masks(LAYER_SEED & 0x7FFFFFFFFFFFFFFF, layer_offsets(LAYER_OFFSET), epoch, LAYER_P, LAYER_P)
