"""The mask decoder over all prompts of an image session as ONE pass (psalm_predictor_forward_batched, PSALM.batch_decoder) on the tiny
architecture with 37 queries, kernels in the host emulation.  The decoder thresholds its own mask logits into the next layer's attention mask, so a
last-bit difference can flip a mask bit and move logits by 1e-2: every comparison with the per-prompt decoder here is word for word."""
import dataclasses

import pytest
import torch

from ops_backend import make_ops
from psalm_amd import hip_ops as H
from psalm_amd.config import PsalmConfig
from psalm_amd.model import PSALM, Instances
from psalm_amd.synthetic import fix_indices, make_state_dict, session_inputs
from session_util import seg_kwargs

Q = 37                                                                    # three query tiles, the last with 5 rows; B * Q is no multiple of 32
SHAPES = [(3, 3), (6, 5), (12, 10)]
_MODELS, _DEC = {}, {}


def _model(task="panoptic", seed=11):
    if task not in _MODELS:
        cfg = dataclasses.replace(PsalmConfig.tiny(task), md_queries=Q)
        sd = make_state_dict(cfg, seed=seed)
        m = PSALM(cfg, sd, ops=make_ops("emu"), precision="f16x3")
        assert m.c_stages and m.batch_decoder is True and m.decoder_batch_max == 8
        _MODELS[task] = (cfg, m)
    return _MODELS[task]


def _decoder_inputs(mf_size):
    """level tokens, mask features and the K / V front psalm_predictor_kv writes for them: computed once per geometry, only read afterwards"""
    if mf_size not in _DEC:
        cfg, m = _model()
        D, MD = cfg.md_hidden, cfg.md_mask_dim
        g = torch.Generator().manual_seed(7 + mf_size[0])
        ms = [torch.randn(h * w, D, generator=g) for h, w in SHAPES]
        mf = torch.randn(mf_size[0] * mf_size[1], MD, generator=g)
        desc, prpos = m._predictor_desc(SHAPES)
        kv = {n: m.ops.predictor_kv(desc, ms, SHAPES, prpos, mf, mf_size, n_reg=n, own=True) for n in (0, 1, 2, 3)}
        _DEC[mf_size] = (ms, mf, desc, prpos, kv)
    return _DEC[mf_size]


def _both_settings(ops, fn):
    try:
        for v in (1, 0):
            ops.set_tuning(ops.TUNE_MHA_QTILE_WAVES, v)
            ops.set_tuning(ops.TUNE_DECODER_FUSE, v)
            fn(v)
    finally:
        ops.set_tuning(ops.TUNE_MHA_QTILE_WAVES, 1)
        ops.set_tuning(ops.TUNE_DECODER_FUSE, 1)


# per-prompt (class, SEG, region) embedding counts of a case
TASKS = {"referring": [(0, 1, 0)] * 3, "panoptic": [(10, 0, 0), (4, 0, 0), (7, 0, 0)], "region": [(0, 0, 1), (0, 0, 3), (0, 0, 2)],
         "all_heads": [(5, 1, 2), (9, 1, 1), (1, 1, 3)]}


SMALL, LARGE = (24, 20), (68, 64)                                         # H2*W2 <= 4096: exact-fp32 mask GEMM; > 4096: split-f16 mask GEMM


@pytest.mark.parametrize("task,B,mf_size", [(t, b, g) for t in ("referring", "panoptic", "region") for b in (1, 3) for g in (SMALL, LARGE)]
                         + [("all_heads", 3, SMALL)])                     # (two heads paired and a third on its own)
def test_batched_stage_is_bitwise_the_per_prompt_loop(task, B, mf_size):
    cfg, m = _model()
    o = m.ops
    D = cfg.md_hidden
    ms, mf, desc, prpos, kv = _decoder_inputs(mf_size)
    counts = TASKS[task][:B]
    g = torch.Generator().manual_seed(B + mf_size[0] + len(task))
    seg_q = torch.randn(B * Q, D, generator=g)
    embs = [torch.randn(sum(c[k] for c in counts), D, generator=g) if any(c[k] for c in counts) else None for k in range(3)]
    front = o.predictor_kv_bytes(desc, SHAPES, mf_size)
    assert 0 < front <= kv[0][2]

    def run(v):
        ws, off, _, _ = kv[0]
        before = ws[off:off + front].clone()
        masks, cls_l, seg_l, reg_l = o.predictor_forward_batched(desc, SHAPES, kv[0], mf, mf_size, seg_q,
                                                                 class_emb=embs[0], cls_counts=[c[0] for c in counts] if embs[0] is not None else None,
                                                                 seg_emb=embs[1], seg_counts=[c[1] for c in counts] if embs[1] is not None else None,
                                                                 region_emb=embs[2], reg_counts=[c[2] for c in counts] if embs[2] is not None else None)
        assert torch.equal(ws[off:off + front], before), "the K / V front is read only"
        packed = [cls_l, seg_l, reg_l]
        offs = [0, 0, 0]
        for b, c in enumerate(counts):
            e = [embs[k][offs[k]:offs[k] + c[k]] if embs[k] is not None else None for k in range(3)]
            w_masks, w_cls, w_seg, w_reg = o.predictor_forward(desc, ms, SHAPES, prpos, mf, mf_size, seg_q[b * Q:(b + 1) * Q], class_emb=e[0], seg_emb=e[1],
                                                               region_emb=e[2], kv=kv[c[2]])
            assert torch.equal(masks[b * Q:(b + 1) * Q], w_masks), (v, b)
            for k, want in enumerate((w_cls, w_seg, w_reg)):
                if want is None:
                    assert packed[k] is None
                    continue
                got = packed[k][Q * offs[k]:Q * (offs[k] + c[k])].view(want.shape)
                assert torch.equal(got, want), (v, b, k)
                offs[k] += c[k]
        for k in range(3):
            assert packed[k] is None or packed[k].numel() == Q * offs[k]

    _both_settings(o, run)


def test_batched_stage_argument_checks():
    cfg, m = _model()
    o = m.ops
    D = cfg.md_hidden
    ms, mf, desc, prpos, kv = _decoder_inputs((24, 20))
    with pytest.raises(H.PsalmHipError, match="psalm_predictor_forward_batched: 1 <= B <= 16 prompts"):
        o.predictor_forward_batched(desc, SHAPES, kv[0], mf, (24, 20), torch.zeros(17 * Q, D))
    with pytest.raises(H.PsalmHipError, match="psalm_predictor_forward_batched: an offset array starts at 0"):
        o.predictor_forward_batched(desc, SHAPES, kv[0], mf, (24, 20), torch.zeros(3 * Q, D), seg_emb=torch.zeros(4, D), offsets={"seg": [1, 2, 3, 4]})
    with pytest.raises(H.PsalmHipError, match="psalm_predictor_forward_batched: offsets do not decrease"):
        o.predictor_forward_batched(desc, SHAPES, kv[0], mf, (24, 20), torch.zeros(3 * Q, D), seg_emb=torch.zeros(4, D), offsets={"seg": [0, 2, 1, 4]})


# ---------------------------------------------------------------------------------------------------------------- session calls
def _same(a, b, path="result"):
    if torch.is_tensor(a):
        assert torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), path
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


def _count_batched(o):
    """wraps Ops.predictor_forward_batched to record the B of every call"""
    calls = []
    real = o.predictor_forward_batched

    def spy(desc, shapes, kv, mf, mf_size, seg_query, **kw):
        calls.append(int(seg_query.shape[0]) // Q)
        return real(desc, shapes, kv, mf, mf_size, seg_query, **kw)

    o.predictor_forward_batched = spy
    return calls


def _segment(m, sess, kw, on, bmax=8, **more):
    m.batch_decoder, m.decoder_batch_max = on, bmax
    try:
        torch.manual_seed(5)                                              # (the region task's point sampler draws from the global generator)
        return m.segment(sess, **kw, **more)
    finally:
        del m.batch_decoder, m.decoder_batch_max                          # back to the class defaults


@pytest.mark.parametrize("task,n,posts", [("referring", 3, (False, True)), ("region", 3, (False,)), ("panoptic", 2, (True,))])
def test_segment_with_the_batched_decoder_is_bitwise_the_loop(task, n, posts):
    cfg, m = _model(task)
    inp = fix_indices(session_inputs(cfg, task, n))
    kw = seg_kwargs(inp)
    sess = m.encode_image(inp["images"][:1], inp["seg_info"][0])
    calls = _count_batched(m.ops)
    try:
        for post in posts:
            kwp = kw if post else {k: v for k, v in kw.items() if k != "is_thing_list"}
            del calls[:]
            off = _segment(m, sess, kwp, False, postprocess=post)
            assert calls == []
            on = _segment(m, sess, kwp, True, postprocess=post)
            assert calls == [n]
            _same(on, off)
            if n == 3:                                                    # a chunk of two prompts and a chunk of one
                del calls[:]
                two = _segment(m, sess, kwp, True, bmax=2, postprocess=post)
                assert calls == [2]
                _same(two, off)
    finally:
        del m.ops.predictor_forward_batched


def test_segment_many_batches_the_prompts_of_a_session():
    """two sessions of different image sizes, the first listed in two requests: its six prompts go through the decoder as ONE batch, the other
    session's two as another; every result equals the per-prompt loop's"""
    cfg, m = _model("referring")
    a = fix_indices(session_inputs(cfg, "referring", 3, size=96, seed=4))
    b = fix_indices(session_inputs(cfg, "referring", 2, size=64, seed=9))
    drop = lambda inp: {k: v for k, v in seg_kwargs(inp).items() if k != "is_thing_list"}      # noqa: E731
    sa, sb = m.encode_image(a["images"][:1], a["seg_info"][0]), m.encode_image(b["images"][:1], b["seg_info"][0])
    assert sa.mask_features_size != sb.mask_features_size
    reqs = [(sa, drop(a)), (sb, drop(b)), (sa, drop(a))]
    calls = _count_batched(m.ops)
    try:
        res = {}
        for on in (False, True):
            m.batch_decoder = on
            for post in (False, True):
                del calls[:]
                res[on, post] = m.segment_many(reqs, postprocess=post)
                assert calls == ([6, 2] if on else [])
    finally:
        del m.batch_decoder, m.ops.predictor_forward_batched
    for post in (False, True):
        assert [len(r) for r in res[True, post]] == [3, 2, 3]
        _same(res[True, post], res[False, post])
