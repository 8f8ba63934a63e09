"""Image sessions on the MI355X: PSALM.segment(PSALM.encode_image(img), prompts) through libpsalm_hip.so vs the CPU oracle's eval_seg on N
copies of the image (tiny architecture, both fp32-class modes) and vs the oracle's predictor outputs on the full-width model."""
import json
import os

import pytest
import torch

from oracle import psalm_oracle as O
from psalm_amd.config import PsalmConfig
from psalm_amd.synthetic import make_state_dict
from session_util import fix_indices, prefix_cache_vs_one_shot, seg_kwargs, session_inputs

pytestmark = pytest.mark.gpu
REPORT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "reports", "parity_report.jsonl")   # git-ignored


def _report(**kw):
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    with open(REPORT, "a") as f:
        f.write(json.dumps(kw) + "\n")


@pytest.mark.parametrize("task,n", [("referring", 3), ("region", 2)])
def test_tiny_session_vs_oracle_on_gpu(task, n):
    """mask_pred within 2e-3 of the oracle's (the bar of test_tiny_vs_oracle_on_gpu), scores / binary masks / gt as tests/test_6_model_emu.py compares them"""
    from psalm_amd.model import PSALM
    cfg = PsalmConfig.tiny(task)
    sd = make_state_dict(cfg, seed=12)
    inp = fix_indices(session_inputs(cfg, task, n))
    torch.manual_seed(5)
    want = O.eval_seg(sd, cfg, **inp)
    if task == "region":
        torch.manual_seed(5)
        _, st = O.eval_seg(sd, cfg, return_stages=True, postprocess=False, **inp)
    for precision in ("f16x3", "fp32"):
        model = PSALM(cfg, sd, precision=precision)
        sess = model.encode_image(inp["images"][:1], inp["seg_info"][0])
        if task == "region":
            # this tiny random model's masks are all negative, so every region SCORE is exactly 0 on both sides and the score comparison below
            # says nothing for this task: the region logits behind the scores are compared too, at the bar tests/test_6_model_emu.py holds
            # forward_logits' pred_region_logits to
            torch.manual_seed(5)
            raw = model.segment(sess, postprocess=False, **{k: v for k, v in seg_kwargs(inp).items() if k != "is_thing_list"})
            for b in range(n):
                wl = st["pred_region_logits"][b]
                el = float((raw[b]["pred_region_logits"].cpu() - wl).abs().max() / wl.abs().max().clamp(min=1e-6))
                print(f"session tiny region {precision} prompt {b}: pred_region_logits err {el:.3e} (max |oracle| {float(wl.abs().max()):.3e})")
                _report(test="session_tiny_region_logits", precision=precision, prompt=b, region_logits_err=el)
                assert float(wl.abs().max()) > 0 and el < 2e-3, (precision, b, el)
        torch.manual_seed(5)
        got = model.segment(sess, **seg_kwargs(inp))
        torch.cuda.synchronize()
        assert len(got) == n and sess.prefix_builds == 1
        for b in range(n):
            a, w = got[b]["mask_pred"].cpu(), want[b]["mask_pred"]
            err = float((a - w).abs().max() / w.abs().max())
            gi, wi = got[b]["instances"], want[b]["instances"]
            if task == "referring":
                sc = float((torch.sort(gi.scores.cpu()).values - torch.sort(wi.scores).values).abs().max())
                gm = torch.zeros_like(wi.pred_masks)
                gm[gi.query_index.cpu()] = gi.pred_masks.cpu()
                wm = torch.zeros_like(wi.pred_masks)
                wm[wi.query_index] = wi.pred_masks
            else:
                # relative as tests/test_6_model_emu.py's _rel: the denominator is floored (this tiny random model's masks can be all negative ->
                # every region score is exactly 0 on both sides)
                sc = float((gi.scores.cpu() - wi.scores).abs().max() / wi.scores.abs().max().clamp(min=1e-6))
                gm, wm = gi.pred_masks.cpu(), wi.pred_masks
                assert float((got[b]["gt"].cpu() - want[b]["gt"]).abs().max()) <= 1e-5 * float(want[b]["gt"].abs().max())
            flips = float((gm != wm).float().mean())
            print(f"session tiny {task} {precision} prompt {b}: mask_pred err {err:.3e}, score err {sc:.3e}, mask flips {flips:.3e}")
            _report(test=f"session_tiny_{task}", precision=precision, prompt=b, mask_pred_err=err, score_err=sc, mask_flips=flips)
            assert err < 2e-3, (precision, err)
            assert sc < (1e-4 if task == "referring" else 2e-3) and flips < 1e-3


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_prefix_pass_cache_vs_one_shot_pass_rows_on_gpu(precision):
    """Every layer's K / V cache of the prefix pass (psalm_phi_prefix; M = P rows) against rows [0, P) of the one-shot pass over three prompts
    (M = B * L rows): RoPE'd K from the prefill kernel's workspace, V from the [k|v|q|fc1] GEMM's v columns.  The GEMMs pick their tile form (and
    split-K) by M, so the two passes may sum in different orders: held to the 3e-5 bound of tests/test_1_ops.py's tol(float32, scale); whether a
    layer came out bitwise is printed and reported."""
    from psalm_amd.model import PSALM
    cfg = PsalmConfig.tiny("referring")
    sd = make_state_dict(cfg, seed=11)
    inp = fix_indices(session_inputs(cfg, "referring", 3, seed=3))
    P, layers = prefix_cache_vs_one_shot(PSALM(cfg, sd, precision=precision), inp)
    assert P >= 1 and len(layers) == cfg.num_layers
    for i, (kc, vc, kr, v) in enumerate(layers):
        dk = max(float((kc - kr[b]).abs().max()) for b in range(kr.shape[0]))
        dv = max(float((vc - v[b]).abs().max()) for b in range(v.shape[0]))
        mk, mv = float(kr.abs().max()), float(v.abs().max())
        print(f"prefix cache vs one-shot {precision} layer {i}: K diff {dk:.3e} (max {mk:.3e}), V diff {dv:.3e} (max {mv:.3e}), bitwise {dk == 0 and dv == 0}")
        _report(test="session_prefix_cache_vs_one_shot", precision=precision, layer=i, k_diff=dk, v_diff=dv, k_max=mk, v_max=mv)
        assert dk <= 3e-5 * mk and dv <= 3e-5 * mv, (i, dk, dv)


_FULL = {}


def _full_case():
    """full-width, 2-layer referring model at 384^2, one image, three sentences: inputs and the CPU oracle's predictor outputs, computed once"""
    if not _FULL:
        cfg = PsalmConfig(num_layers=2, seg_task="referring")
        sd = make_state_dict(cfg, seed=SEED)
        inp = fix_indices(session_inputs(cfg, "referring", 3, size=384, seed=SEED))
        torch.manual_seed(5)
        _, st = O.eval_seg(sd, cfg, return_stages=True, postprocess=False, **inp)
        _FULL.update(cfg=cfg, sd=sd, inp=inp, st=st)
    return _FULL


SEED = 3


def test_full_width_session_vs_oracle():
    """pred_masks and pred_SEG_logits of the session path within 1e-3 of max|oracle| (what tests/test_9_e2e_gpu.py holds the fp32-class modes to
    against the reference-generated goldens).  Model / input seed 3; for this seed the CPU oracle against itself at 1 vs 8 host threads differs
    by at most 1.5e-6 (pred_masks) / 1.2e-6 (pred_SEG_logits) of max|oracle| over the three prompts: three orders inside the bar."""
    from psalm_amd.model import PSALM
    c = _full_case()
    cfg, inp, st = c["cfg"], c["inp"], c["st"]
    model = PSALM(cfg, c["sd"], precision="f16x3")
    sess = model.encode_image(inp["images"][:1], inp["seg_info"][0])
    outs = model.segment(sess, postprocess=False, **seg_kwargs(inp))
    torch.cuda.synchronize()
    for b, o in enumerate(outs):
        wm, ws = st["pred_masks"][b], st["pred_SEG_logits"][b]
        em = float((o["pred_masks"].cpu() - wm).abs().max() / wm.abs().max())
        es = float((o["pred_SEG_logits"].cpu() - ws).abs().max() / ws.abs().max())
        print(f"session full-width prompt {b}: pred_masks err {em:.3e}, pred_SEG_logits err {es:.3e}")
        _report(test="session_full_width_referring_384", precision="f16x3", prompt=b, pred_masks_err=em, seg_logits_err=es)
        assert em < 1e-3 and es < 1e-3, (b, em, es)
    _FULL["model"], _FULL["sess"] = model, sess


def test_session_is_deterministic_without_graphs():
    """the same segment call twice (second one on the cached prefix): bitwise-equal outputs"""
    from psalm_amd.model import PSALM
    c = _full_case()
    inp = c["inp"]
    model = c.get("model") or PSALM(c["cfg"], c["sd"], precision="f16x3")
    sess = c.get("sess") or model.encode_image(inp["images"][:1], inp["seg_info"][0])
    a = model.segment(sess, postprocess=False, **seg_kwargs(inp))
    b = model.segment(sess, postprocess=False, **seg_kwargs(inp))
    torch.cuda.synchronize()
    assert sess.prefix_hits >= 1
    for x, y in zip(a, b):
        assert torch.equal(x["pred_masks"], y["pred_masks"]) and torch.equal(x["pred_SEG_logits"], y["pred_SEG_logits"])
