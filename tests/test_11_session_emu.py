"""Image sessions (PSALM.encode_image / PSALM.segment: encode once, segment many prompts) on the tiny architecture, kernels in the host
emulation, against the CPU oracle's eval_seg on N copies of the image.  The bars are those tests/test_6_model_emu.py applies to eval_seg in
the same precision."""
import pytest
import torch

from ops_backend import make_ops
from oracle import psalm_oracle as O
from psalm_amd.config import PsalmConfig
from psalm_amd.model import PSALM, ImageSession
from psalm_amd.synthetic import make_state_dict
from session_util import fix_indices as _fix_indices, prefix_cache_vs_one_shot, seg_kwargs, session_inputs


def _rel(a, b):
    return ((a.float().cpu() - b.float()).abs().max() / b.float().abs().max().clamp(min=1e-6)).item()


def _compare_f16x3_panoptic(g, w):
    """the assertions of test_6_model_emu.py::test_tiny_eval_seg_f16x3_mode on its eval_seg result, unchanged"""
    assert _rel(g["mask_pred"], w["mask_pred"]) < 1e-4
    assert _rel(g["sem_seg"], w["sem_seg"]) < 1e-4
    # labels: identical wherever the oracle's decision is not an exact tie (see test_6: this tiny random model has pixels whose two best classes
    # differ by less than one fp32 ulp of the sum)
    top2 = w["sem_seg"].topk(2, 0).values
    decided = (top2[0] - top2[1]) > 1e-6 * w["sem_seg"].abs().max()
    same = g["sem_seg"].argmax(0).cpu() == w["sem_seg"].argmax(0)
    assert bool(same[decided].all()) and same.float().mean() >= 0.98
    assert torch.equal(g["panoptic_seg"][0].cpu(), w["panoptic_seg"][0])
    assert g["panoptic_seg"][1] == w["panoptic_seg"][1]
    gi, wi = g["instances"], w["instances"]
    assert len(gi.scores) == len(wi.scores)
    assert (torch.sort(gi.scores.cpu()).values - torch.sort(wi.scores).values).abs().max() < 1e-4


def _compare(task, g, w):
    """the assertions of test_6_model_emu.py::test_tiny_eval_seg_postprocess_fp32 on one eval_seg result, unchanged (test_6 has no f16x3 case for
    referring / region; it holds that mode to "the tolerances of the fp32-mode tests", i.e. these)"""
    assert _rel(g["mask_pred"], w["mask_pred"]) < 2e-3
    gi, wi = g["instances"], w["instances"]
    if task == "panoptic":
        assert (g["sem_seg"].argmax(0).cpu() == w["sem_seg"].argmax(0)).float().mean() > 0.999
        assert _rel(g["sem_seg"], w["sem_seg"]) < 2e-3
        gp, ginfo = g["panoptic_seg"]
        wp, winfo = w["panoptic_seg"]
        assert ginfo == winfo
        assert (gp.cpu() == wp).float().mean() > 0.999
        og = sorted(zip((-gi.scores.cpu()).tolist(), gi.pred_classes.cpu().tolist()))
        ow = sorted(zip((-wi.scores).tolist(), wi.pred_classes.tolist()))
        assert len(og) == len(ow)
        for (a, c1), (b_, c2) in zip(og, ow):
            assert abs(a - b_) < 1e-4 and c1 == c2
    elif task == "referring":
        assert (torch.sort(gi.scores.cpu()).values - torch.sort(wi.scores).values).abs().max() < 1e-4
        gm = torch.zeros_like(wi.pred_masks)
        gm[gi.query_index.cpu()] = gi.pred_masks.cpu()
        wm = torch.zeros_like(wi.pred_masks)
        wm[wi.query_index] = wi.pred_masks
        assert (gm != wm).float().mean() < 1e-3
    else:
        assert _rel(gi.scores, wi.scores) < 2e-3
        assert (gi.pred_masks.cpu() != wi.pred_masks).float().mean() < 1e-3
        assert _rel(g["gt"], w["gt"]) < 1e-5


_MODELS = {}


def _model(task, precision, seed=12):
    key = (task, precision, seed)
    if key not in _MODELS:
        cfg = PsalmConfig.tiny(task)
        sd = make_state_dict(cfg, seed=seed)
        _MODELS[key] = (cfg, sd, PSALM(cfg, sd, ops=make_ops("emu"), precision=precision))
    return _MODELS[key]


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("task,n", [("referring", 3), ("region", 2), ("panoptic", 1)])
def test_segment_vs_oracle_eval_seg_on_copies(task, n, precision):
    """segment(encode_image(img), prompts) == the oracle's eval_seg on n copies of the image (referring: three sentences of different lengths; region:
    prompts with 1 and 3 regions), same keys / dtypes as the model's own eval_seg."""
    cfg, sd, model = _model(task, precision)
    inp = _fix_indices(session_inputs(cfg, task, n))
    torch.manual_seed(5)
    want = O.eval_seg(sd, cfg, **inp)
    sess = model.encode_image(inp["images"][:1], inp["seg_info"][0])
    assert isinstance(sess, ImageSession) and sess.prefix_cache is None and sess.prefix_builds == 0
    torch.manual_seed(5)
    got = model.segment(sess, **seg_kwargs(inp))
    assert len(got) == n and sess.prefix_builds == 1
    for b in range(n):
        if precision == "f16x3" and task == "panoptic":
            _compare_f16x3_panoptic(got[b], want[b])
        else:
            _compare(task, got[b], want[b])
    if precision != "fp32":                    # (keys / dtypes / shapes / devices against the model's own eval_seg: once, in the cheaper mode on the emulator)
        return
    torch.manual_seed(5)
    own = model.eval_seg(**inp)
    for b in range(n):
        assert set(got[b]) == set(own[b])
        for k, v in own[b].items():
            if torch.is_tensor(v):
                assert got[b][k].dtype == v.dtype and got[b][k].shape == v.shape and got[b][k].device == v.device, k


def test_session_vision_tensors_are_bitwise_the_one_shot_ones():
    cfg, sd, model = _model("referring", "f16x3")
    inp = _fix_indices(session_inputs(cfg, "referring", 1))
    st = {}
    model.forward_logits(stages=st, **{k: v for k, v in inp.items() if k != "is_thing_list"})
    sess = model.encode_image(inp["images"][0], inp["seg_info"])
    for (ta, ha, wa), (tb, hb, wb) in zip(sess.feats, st["feats"]):
        assert (ha, wa) == (hb, wb) and torch.equal(ta, tb)
    assert torch.equal(sess.image_tokens, st["image_tokens"])
    assert torch.equal(sess.mask_features, st["mask_features"][0])
    assert all(torch.equal(a, b) for a, b in zip(sess.multi_scale_features, st["multi_scale_features"][0]))
    assert sess.nbytes() > 0


@pytest.mark.parametrize("task,n", [("referring", 3), ("region", 2)])
def test_session_stage_calls_are_bitwise_the_op_by_op_sequence(task, n):
    """psalm_phi_prefix + psalm_phi_suffix (one native call each) == PSALM._llm_session's op-by-op sequence: cache, hidden states and predictor outputs."""
    cfg, sd, m = _model(task, "f16x3", seed=11)
    kw = seg_kwargs(_fix_indices(session_inputs(cfg, task, n, seed=3)))
    img = session_inputs(cfg, task, n, seed=3)["images"][:1]
    assert m.c_stages
    m._cache.pop(("phi_desc",), None)
    sa, sb = {}, {}
    s1 = m.encode_image(img)
    torch.manual_seed(77)
    oa = m.segment(s1, postprocess=False, stages=sa, **kw)
    assert ("phi_desc",) in m._cache                              # the stage-level calls ran (the op-by-op branch never builds the descriptor)
    m.c_stages = False
    try:
        s2 = m.encode_image(img)
        torch.manual_seed(77)
        ob = m.segment(s2, postprocess=False, stages=sb, **kw)
    finally:
        m.c_stages = True
    for (ka, va), (kb, vb) in zip(s1.prefix_cache[1], s2.prefix_cache[1]):      # per layer: RoPE'd K (heads, ceil32 P, 64), V (P, hidden)
        assert torch.equal(ka, kb) and torch.equal(va, vb)
    assert torch.equal(sa["hidden_states"], sb["hidden_states"])
    for a, b in zip(oa, ob):
        assert torch.equal(a["pred_masks"], b["pred_masks"])
        for k in ("pred_class_name_logits", "pred_SEG_logits", "pred_region_logits"):
            assert (a[k] is None) == (b[k] is None) and (a[k] is None or torch.equal(a[k], b[k])), k


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_prefix_pass_cache_is_the_one_shot_pass_rows(precision):
    """Every layer's K / V cache written by the prefix pass (psalm_phi_prefix in f16x3, the op sequence in fp32; M = P rows) against what the ONE-SHOT pass
    over three prompts (M = B * L rows) holds for rows [0, P) of each prompt: K = phi_rope_prep_f32_kernel's output in the prefill kernel's
    workspace, V = the [k|v|q|fc1] GEMM's v columns.
    f16x3: bitwise in every layer -- the split-f16 GEMM takes the same form for M = P as for M = B * L, and the row scales of the hand-over to
    [dense|fc2] (a maximum over the rows of the call, so over other rows in the two passes) come out equal.
    fp32: NOT bitwise on the emulator -- the fp32 GEMM sums K in another order for M = P = 8 than for M = B * L (measured: K 2.7e-6, V 3.9e-6 at
    max |.| 3.4 / 3.9, i.e. 1e-6 relative) -- so that mode is held to the 3e-5 bound of tests/test_1_ops.py's tol(float32, scale) instead."""
    cfg, sd, m = _model("referring", precision, seed=11)
    inp = _fix_indices(session_inputs(cfg, "referring", 3, seed=3))
    P, layers = prefix_cache_vs_one_shot(m, inp)
    assert P >= 1 and len(layers) == cfg.num_layers >= 2
    for i, (kc, vc, kr, v) in enumerate(layers):
        for b in range(kr.shape[0]):
            dk, dv = float((kc - kr[b]).abs().max()), float((vc - v[b]).abs().max())
            print(f"{precision} layer {i} prompt {b}: K diff {dk:.3e} (max {float(kr[b].abs().max()):.3e}), V diff {dv:.3e} (max {float(v[b].abs().max()):.3e})")
            if precision == "f16x3":
                assert torch.equal(kc, kr[b]) and torch.equal(vc, v[b]), (i, b, dk, dv)
            else:
                assert dk <= 3e-5 * float(kr[b].abs().max()) and dv <= 3e-5 * float(v[b].abs().max()), (i, b, dk, dv)


def test_second_segment_reuses_the_prefix_cache():
    cfg, sd, model = _model("referring", "f16x3")
    inp = _fix_indices(session_inputs(cfg, "referring", 3))
    kw = seg_kwargs(inp)
    one = lambda b: {k: (v[b:b + 1] if k != "is_thing_list" else v) for k, v in kw.items()}      # noqa: E731
    sess = model.encode_image(inp["images"][:1], inp["seg_info"][0])
    model.segment(sess, **one(0))
    assert (sess.prefix_builds, sess.prefix_hits) == (1, 0)
    second = model.segment(sess, **one(1))[0]
    assert (sess.prefix_builds, sess.prefix_hits) == (1, 1)
    fresh = model.segment(model.encode_image(inp["images"][:1], inp["seg_info"][0]), **one(1))[0]
    assert torch.equal(second["mask_pred"], fresh["mask_pred"])
    assert torch.equal(second["instances"].scores, fresh["instances"].scores)
    assert torch.equal(second["instances"].pred_masks, fresh["instances"].pred_masks)
    # another leading text: the cache is rebuilt, not reused
    other = one(2)
    other["input_ids"] = other["input_ids"].clone()
    other["input_ids"][0, 0] = (int(other["input_ids"][0, 0]) + 1) % cfg.vocab_size
    model.segment(sess, **other)
    assert (sess.prefix_builds, sess.prefix_hits) == (2, 1)


def test_session_errors():
    cfg, sd, model = _model("referring", "f16x3")
    inp = _fix_indices(session_inputs(cfg, "referring", 2))
    kw = seg_kwargs(inp)
    sess = model.encode_image(inp["images"][:1], inp["seg_info"][0])
    bad = dict(kw)
    bad["input_ids"] = kw["input_ids"].clone()
    bad["input_ids"][1, 2] = (int(bad["input_ids"][1, 2]) + 1) % cfg.vocab_size
    with pytest.raises(ValueError, match="token position 2"):
        model.segment(sess, **bad)
    with pytest.raises(NotImplementedError):
        PSALM(cfg, sd, ops=make_ops("emu"), precision="bf16").encode_image(inp["images"][:1])
    with pytest.raises(NotImplementedError):
        PSALM(cfg, sd, ops=make_ops("emu"), precision="f16x3", llm_products=1).encode_image(inp["images"][:1])
    other = PSALM(cfg, sd, ops=make_ops("emu"), precision="f16x3")
    with pytest.raises(ValueError, match="another model"):
        other.segment(sess, **kw)
    with pytest.raises(ValueError, match="another model"):
        model.replica().segment(sess, **kw)
    rep = model.replica()
    rsess = rep.encode_image(inp["images"][:1], inp["seg_info"][0])
    model._prepare_weights(sd)                                    # weights prepared again: live sessions are stale, a replica's too (shared weights)
    try:
        with pytest.raises(ValueError, match="prepared again"):
            model.segment(sess, **kw)
        with pytest.raises(ValueError, match="prepared again"):
            rep.segment(rsess, **kw)
    finally:
        _MODELS.clear()
