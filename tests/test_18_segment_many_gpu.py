"""PSALM.segment_many on the MI355X: prompts on two images in one Phi suffix pass through libpsalm_hip.so, against the CPU oracle's eval_seg per
image, against PSALM.segment, and twice for determinism (tiny architecture, precision f16x3)."""
import pytest
import torch

from grouped_util import encode_pair, prefix_lengths, referring_pair, requests
from oracle import psalm_oracle as O
from psalm_amd.config import PsalmConfig
from psalm_amd.synthetic import make_state_dict

pytestmark = pytest.mark.gpu

_CASE = {}


def _case():
    """model, inputs, sessions and one segment_many result, computed once and shared"""
    if not _CASE:
        from psalm_amd.model import PSALM
        cfg = PsalmConfig.tiny("referring")
        sd = make_state_dict(cfg, seed=12)
        pair = referring_pair(cfg)
        model = PSALM(cfg, sd, precision="f16x3")
        sessions = encode_pair(model, pair)
        got = model.segment_many(requests(sessions, pair))
        torch.cuda.synchronize()
        _CASE.update(cfg=cfg, sd=sd, pair=pair, model=model, sessions=sessions, got=got)
    return _CASE


def test_tiny_segment_many_vs_oracle_on_gpu():
    """tests/test_12_session_gpu.py::test_tiny_session_vs_oracle_on_gpu's referring assertions, per prompt of each image"""
    c = _case()
    torch.manual_seed(5)
    want = [O.eval_seg(c["sd"], c["cfg"], **inp) for inp in c["pair"]]
    Ps, tiles = prefix_lengths(c["sessions"])
    print(f"prefix lengths {Ps}, in different 32-row key tiles: {tiles}")
    assert [len(g) for g in c["got"]] == [3, 2] and all(s.prefix_builds == 1 for s in c["sessions"])
    for r, (gr, wr) in enumerate(zip(c["got"], want)):
        for b, (g, w_) in enumerate(zip(gr, wr)):
            a, w = g["mask_pred"].cpu(), w_["mask_pred"]
            err = float((a - w).abs().max() / w.abs().max())
            gi, wi = g["instances"], w_["instances"]
            sc = float((torch.sort(gi.scores.cpu()).values - torch.sort(wi.scores).values).abs().max())
            gm = torch.zeros_like(wi.pred_masks)
            gm[gi.query_index.cpu()] = gi.pred_masks.cpu()
            wm = torch.zeros_like(wi.pred_masks)
            wm[wi.query_index] = wi.pred_masks
            flips = float((gm != wm).float().mean())
            print(f"segment_many tiny referring f16x3 image {r} prompt {b}: mask_pred err {err:.3e}, score err {sc:.3e}, mask flips {flips:.3e}")
            assert err < 2e-3, (r, b, err)
            assert sc < 1e-4 and flips < 1e-3


def test_single_request_is_bitwise_segment_on_gpu():
    c = _case()
    model, pair = c["model"], c["pair"]
    (sess, kw), = requests(encode_pair(model, pair[:1]), pair[:1])
    got = model.segment_many([(sess, kw)], postprocess=False)[0]
    want = model.segment(model.encode_image(pair[0]["images"][:1], pair[0]["seg_info"][0]), postprocess=False, **kw)
    torch.cuda.synchronize()
    assert len(got) == len(want) == 3
    for a, b in zip(got, want):
        assert torch.equal(a["pred_masks"], b["pred_masks"]) and torch.equal(a["pred_SEG_logits"], b["pred_SEG_logits"])
    full = model.segment_many([(sess, kw)])[0]
    ref = model.segment(sess, **kw)
    for a, b in zip(full, ref):
        assert torch.equal(a["mask_pred"], b["mask_pred"]) and torch.equal(a["instances"].scores, b["instances"].scores)
        assert torch.equal(a["instances"].pred_masks, b["instances"].pred_masks)


def test_segment_many_is_deterministic_without_graphs():
    """the same call twice (second one on the cached prefixes): bitwise-equal outputs"""
    c = _case()
    again = c["model"].segment_many(requests(c["sessions"], c["pair"]))
    torch.cuda.synchronize()
    assert all(s.prefix_hits >= 1 for s in c["sessions"])
    for gr, hr in zip(c["got"], again):
        for g, h in zip(gr, hr):
            assert torch.equal(g["mask_pred"], h["mask_pred"]) and torch.equal(g["instances"].scores, h["instances"].scores)
            assert torch.equal(g["instances"].pred_masks, h["instances"].pred_masks)
