"""GPU: the vertex-displacement terms WITH gradient in the trainer (LatentPriorLosses(vtex_grad=True), amuse_amd/body.py VertexLossFn): the gradient that reaches the
decoder's output is the vtex_grad=False run's plus LAMBDA_REC / (B F V 3) x amuse_body_vertex_loss_grad's; a captured step replays to the eager step's flat
gradient bit for bit (every kernel involved is deterministic); the trainer's own HIP graphs replay with new batches."""
import numpy as np
import pytest
import torch

import body_cases as bc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ATTR = [("scott", "male"), ("miranda", "female")]


def _models():
    from amuse_amd import body
    return {g: body.BodyModel.from_dict(bc.make_model(203, seed=40 + i)) for i, g in enumerate(("male", "female"))}


def test_trainer_vertex_terms_with_gradient():
    from amuse_amd import body
    from amuse_amd.train_gesture import build_trainer, synthetic_batch
    models = _models()
    batch = dict(synthetic_batch(2, 3, DEV), ld_attr=ATTR)
    g = torch.Generator().manual_seed(0)
    draws = dict(noise=torch.randn(2, 1, 128, generator=g).to(DEV), timesteps=torch.randint(0, 1000, (2,), generator=g).to(DEV),
                 eps_enc=torch.randn(1, 2, 128, generator=g).to(DEV), eps_inf=torch.randn(1, 2, 128, generator=g).to(DEV))
    seen, flat, keep = {}, {}, {}
    for vg in (True, False):
        bl = body.BodyLosses(models, DEV, "v0", grad=vg)
        torch.manual_seed(7)
        tr = build_trainer(DEV, seed=2, dropout=0.0, body=bl, vtex_grad=vg, grads_mode="sink", use_hip_sampler=False)
        inner = bl.terms

        def spy(m_ref, m_rst, gen, attr_, subjects, inner=inner, vg=vg, **kw):
            seen[vg] = dict(ref=m_ref.detach().clone(), rst=m_rst.detach().clone(), kw=dict(kw))
            m_rst.register_hook(lambda gr, vg=vg: seen[vg].__setitem__("grad", gr.detach().clone()))
            return inner(m_ref, m_rst, gen, attr_, subjects, **kw)
        bl.terms = spy
        for m in tr.model.values():
            m.train()
        loss = tr.forward_losses(batch, **draws)
        tr.backward_into_bucket(loss)
        torch.cuda.synchronize()
        bl.terms = inner
        flat[vg], keep[vg] = tr.flat_grad.clone(), (tr, bl, loss.detach().clone())
    assert seen[True]["kw"] == {"grad": True} and seen[False]["kw"] == {}
    assert torch.equal(seen[True]["rst"], seen[False]["rst"]) and torch.equal(keep[True][2], keep[False][2])     # the same step, the same value of the loss
    tr, bl, _ = keep[True]
    B, F, V = 2, int(seen[True]["rst"].shape[1]), 203
    subs = bl.subjects(ATTR)
    buf = torch.zeros_like(seen[True]["rst"])
    for i, gname in enumerate(bl.genders):
        bl.engines[gname].vertex_loss_grad(seen[True]["ref"].contiguous(), seen[True]["rst"].contiguous(), None, subs[i], out=(buf, None))
    assert float(buf[0].abs().max()) > 0 and float(buf[1].abs().max()) > 0                                       # both engines wrote their own clip's rows
    extra = buf * np.float32(tr.lpdm_losses.cfg["LAMBDA_REC"] / float(B * F * V * 3))
    on, off = seen[True]["grad"], seen[False]["grad"]
    err = float((on - (off + extra)).abs().max())
    bar = 4 * 2.0 ** -24 * float(on.abs().max())                                                                 # fp32 round-off of the sum and of the scale
    print(f"hook on feats_rst: |on - (off + term)| {err:.3e} bar {bar:.3e}; term's max {float(extra.abs().max()):.3e} of {float(on.abs().max()):.3e}")
    assert float(extra.abs().max()) > 16 * bar and err <= bar
    assert not torch.equal(flat[True], flat[False])                                                              # ... and it reaches the parameters
    # captured: the same step (explicit draws, dropout 0) replays to the eager flat gradient, bit for bit
    static = dict(batch, ld_subjects=subs)
    for e in bl.engines.values():
        e.reserve(B * F)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    count0 = tr.lpdm_losses.count
    with torch.cuda.graph(graph):
        loss = tr.forward_losses(static, **draws)
        tr.backward_into_bucket(loss)
    tr.lpdm_losses.count = count0
    tr.flat_grad.fill_(7.0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(tr.flat_grad, flat[True])
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(tr.flat_grad, flat[True])
    for _, b, _ in keep.values():
        b.close()


def test_trainer_graphs_replay_with_vertex_gradient():
    """GestureTrainer.enable_graph with vtex_grad: enable_grad + reserve happen before the capture; three replays with new batches give finite losses"""
    from amuse_amd import body
    from amuse_amd.train_gesture import build_trainer, synthetic_batch
    bl = body.BodyLosses(_models(), DEV, "v0", grad=True)
    tr = build_trainer(DEV, seed=2, body=bl, vtex_grad=True)
    batches = [dict(synthetic_batch(2, 10 + i, DEV), ld_attr=ATTR if i % 2 == 0 else ATTR[::-1]) for i in range(4)]
    for i in range(3):
        tr.train_step(batches[i])
    assert tr.enable_graph(batches[0]) and all(e.info()["grad"] == 1 for e in bl.engines.values())
    p0 = tr.flat_param.clone()
    for i in range(3):
        tr.lpdm_losses.reset()
        loss = tr.train_step(batches[1 + i])
        torch.cuda.synchronize()
        assert tr._graph is not None and np.isfinite(float(loss)) and float(tr.lpdm_losses.sums["rec_vtex_displacement"]) > 0
    assert bool(torch.isfinite(tr.flat_param).all()) and not torch.equal(tr.flat_param, p0)
    bl.close()
