"""PSALM.segment_many (prompts on several images in ONE Phi suffix pass through the grouped prefix attention) on the tiny architecture, kernels in
the host emulation: against the CPU oracle's eval_seg on copies of each image, against PSALM.segment, and the stage entry against the op-by-op
sequence.  The bars are those tests/test_11_session_emu.py applies to PSALM.segment."""
import pytest
import torch

from grouped_util import encode_pair, prefix_lengths, referring_pair, region_pair, requests
from ops_backend import make_ops
from oracle import psalm_oracle as O
from psalm_amd.config import PsalmConfig
from psalm_amd.model import PSALM, Instances
from psalm_amd.synthetic import make_state_dict


def _rel(a, b):
    return ((a.float().cpu() - b.float()).abs().max() / b.float().abs().max().clamp(min=1e-6)).item()


def _compare(task, g, w):
    """tests/test_11_session_emu.py::_compare (= test_6_model_emu.py::test_tiny_eval_seg_postprocess_fp32's assertions) for the two tasks used here, unchanged"""
    assert _rel(g["mask_pred"], w["mask_pred"]) < 2e-3
    gi, wi = g["instances"], w["instances"]
    if task == "referring":
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
_WANT = {}


def _model(task, precision, seed=12):
    key = (task, precision, seed)
    if key not in _MODELS:
        cfg = PsalmConfig.tiny(task)
        sd = make_state_dict(cfg, seed=seed)
        _MODELS[key] = (cfg, sd, PSALM(cfg, sd, ops=make_ops("emu"), precision=precision))
    return _MODELS[key]


def _oracle(task, cfg, sd, pair):
    """the oracle's results per image, computed once per task: one RNG seed, images in request order (the order segment_many's region sampler draws in)"""
    if task not in _WANT:
        torch.manual_seed(5)
        _WANT[task] = [O.eval_seg(sd, cfg, **inp) for inp in pair]
    return _WANT[task]


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("task", ["referring", "region"])
def test_segment_many_vs_oracle_eval_seg_per_image(task, precision):
    cfg, sd, model = _model(task, precision)
    pair = (referring_pair if task == "referring" else region_pair)(cfg)
    want = _oracle(task, cfg, sd, pair)
    sessions = encode_pair(model, pair)
    torch.manual_seed(5)
    got = model.segment_many(requests(sessions, pair, drop=()))
    assert [len(g) for g in got] == [inp["input_ids"].shape[0] for inp in pair]
    assert all((s.prefix_builds, s.prefix_hits) == (1, 0) for s in sessions)
    if task == "referring":
        Ps, tiles = prefix_lengths(sessions)
        print(f"prefix lengths {Ps}, in different 32-row key tiles: {tiles}")
    for gr, wr in zip(got, want):
        for g, w in zip(gr, wr):
            _compare(task, g, w)


def _same(a, b, path="result"):
    if torch.is_tensor(a):
        assert torch.is_tensor(b) and a.dtype == b.dtype and torch.equal(a, b), path
    elif isinstance(a, Instances):
        fa, fb = a.get_fields(), b.get_fields()
        assert set(fa) == set(fb), path
        for k in fa:
            _same(fa[k], fb[k], f"{path}.{k}")
    elif isinstance(a, dict):
        assert set(a) == set(b), path
        for k in a:
            _same(a[k], b[k], f"{path}[{k}]")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{path}[{i}]")
    else:
        assert a == b, path


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_single_request_is_bitwise_segment(precision):
    """one group: the grouped pass runs the same rows, the same GEMM shapes and the same scale maxima as segment's"""
    cfg, sd, model = _model("referring", precision)
    pair = referring_pair(cfg)
    (sess, kw), = requests(encode_pair(model, pair[:1]), pair[:1])
    got = model.segment_many([(sess, kw)])
    assert len(got) == 1 and len(got[0]) == 3
    want = model.segment(model.encode_image(pair[0]["images"][:1], pair[0]["seg_info"][0]), **kw)
    _same(got[0], want)


@pytest.mark.parametrize("task", ["referring", "region"])
def test_grouped_stage_call_is_bitwise_the_op_by_op_sequence(task):
    """psalm_phi_suffix_grouped (one native call) == _llm_session's op-by-op sequence with the grouped attention ops: hidden states and predictor
    outputs, two sessions (the pattern of test_session_stage_calls_are_bitwise_the_op_by_op_sequence)"""
    cfg, sd, m = _model(task, "f16x3", seed=11)
    pair = (referring_pair if task == "referring" else region_pair)(cfg)
    assert m.c_stages
    m._cache.pop(("phi_desc",), None)
    sa, sb = {}, {}
    torch.manual_seed(77)
    oa = m.segment_many(requests(encode_pair(m, pair), pair), postprocess=False, stages=sa)
    assert ("phi_desc",) in m._cache                              # the stage-level calls ran (the op-by-op branch never builds the descriptor)
    m.c_stages = False
    try:
        torch.manual_seed(77)
        ob = m.segment_many(requests(encode_pair(m, pair), pair), postprocess=False, stages=sb)
    finally:
        m.c_stages = True
    assert sa["prefix_lens"] == sb["prefix_lens"] and torch.equal(sa["hidden_states"], sb["hidden_states"])
    for ra, rb in zip(oa, ob):
        for a, b in zip(ra, rb):
            assert torch.equal(a["pred_masks"], b["pred_masks"])
            for k in ("pred_class_name_logits", "pred_SEG_logits", "pred_region_logits"):
                assert (a[k] is None) == (b[k] is None) and (a[k] is None or torch.equal(a[k], b[k])), k


def test_cache_accounting():
    cfg, sd, model = _model("referring", "f16x3")
    pair = referring_pair(cfg)
    sessions = encode_pair(model, pair)
    reqs = requests(sessions, pair)
    first = model.segment_many(reqs)
    assert all((s.prefix_builds, s.prefix_hits) == (1, 0) for s in sessions)
    second = model.segment_many(reqs)
    assert all((s.prefix_builds, s.prefix_hits) == (1, 1) for s in sessions)
    _same(first, second)
    # a session listed twice in one call: one cache, built once; each request's answers are those of the request alone
    sess, = encode_pair(model, pair[:1])
    kw = reqs[0][1]
    one = lambda b: {k: v[b:b + 1] for k, v in kw.items()}        # noqa: E731
    twice = model.segment_many([(sess, one(0)), (sess, one(2))])
    assert sess.prefix_builds == 1 and [len(t) for t in twice] == [1, 1]
    other = dict(one(1))
    other["input_ids"] = other["input_ids"].clone()
    other["input_ids"][0, 0] = (int(other["input_ids"][0, 0]) + 1) % cfg.vocab_size
    with pytest.raises(ValueError, match="share a session"):
        model.segment_many([(sess, one(0)), (sess, other)])


def test_segment_many_errors():
    cfg, sd, model = _model("referring", "f16x3")
    pair = referring_pair(cfg)
    sessions = encode_pair(model, pair)
    reqs = requests(sessions, pair)
    with pytest.raises(ValueError, match="empty"):
        model.segment_many([])
    other = PSALM(cfg, sd, ops=make_ops("emu"), precision="f16x3")
    with pytest.raises(ValueError, match="request 1.*another model"):
        model.segment_many([reqs[0], (other.encode_image(pair[1]["images"][:1]), reqs[1][1])])
    bad = dict(reqs[1][1])
    bad["input_ids"] = bad["input_ids"].clone()
    bad["input_ids"][1, 1] = (int(bad["input_ids"][1, 1]) + 1) % cfg.vocab_size
    with pytest.raises(ValueError, match="request 1.*token position 1"):
        model.segment_many([reqs[0], (sessions[1], bad)])
    with pytest.raises(NotImplementedError):
        PSALM(cfg, sd, ops=make_ops("emu"), precision="bf16").segment_many(reqs)
    with pytest.raises(NotImplementedError):
        PSALM(cfg, sd, ops=make_ops("emu"), precision="f16x3", llm_products=1).segment_many(reqs)
