"""The batched mask decoder (psalm_predictor_forward_batched, PSALM.batch_decoder) on the MI355X at the full decoder width -- D 256, 8 heads, 100
queries, 9 layers, three levels, mask_dim 256 -- behind the tiny Phi / Swin: every prompt's outputs equal, word for word, what the per-prompt call
returns for it alone."""
import dataclasses

import pytest
import torch

from psalm_amd.config import PsalmConfig
from psalm_amd.synthetic import fix_indices, make_state_dict, session_inputs
from session_util import seg_kwargs

pytestmark = pytest.mark.gpu

_M = {}
# (mask features, levels) of the benchmark geometries: strides 4 and 32 / 16 / 8
GEOM = {384: ((96, 96), [(12, 12), (24, 24), (48, 48)]), 640: ((160, 160), [(20, 20), (40, 40), (80, 80)]), 1024: ((256, 256), [(32, 32), (64, 64), (128, 128)])}


def _model(**kw):
    key = tuple(sorted(kw.items()))
    if key not in _M:
        from psalm_amd.model import PSALM
        full = dict(md_hidden=256, md_queries=100, md_heads=8, md_dim_ff=2048, md_dec_layers=9, md_mask_dim=256, md_gn_groups=32)
        full.update(kw)
        cfg = dataclasses.replace(PsalmConfig.tiny("referring"), **full)
        m = PSALM(cfg, make_state_dict(cfg, seed=11), precision="f16x3", use_graphs=False)
        assert m.c_stages and m.batch_decoder is True
        _M[key] = (cfg, m)
    return _M[key]


def _stage_vs_loop(cfg, m, mf_size, shapes, B, counts):
    """psalm_predictor_forward_batched against a loop of psalm_predictor_forward(kv_ready = 1) on one K / V front; counts: per prompt (class, SEG)"""
    o = m.ops
    D, Q, MD = cfg.md_hidden, cfg.md_queries, cfg.md_mask_dim
    g = torch.Generator().manual_seed(B + mf_size[0])
    d = o.device
    ms = [torch.randn(h * w, D, generator=g).to(d) for h, w in shapes]
    mf = torch.randn(mf_size[0] * mf_size[1], MD, generator=g).to(d)
    seg_q = torch.randn(B * Q, D, generator=g).to(d)
    embs = [torch.randn(sum(c[k] for c in counts), D, generator=g).to(d) for k in range(2)]
    desc, prpos = m._predictor_desc(shapes)
    kv = o.predictor_kv(desc, ms, shapes, prpos, mf, mf_size, n_reg=0, own=True)
    front = o.predictor_kv_bytes(desc, shapes, mf_size)
    before = kv[0][kv[1]:kv[1] + front].clone()
    masks, cls_l, seg_l, _ = o.predictor_forward_batched(desc, shapes, kv, mf, mf_size, seg_q, class_emb=embs[0], cls_counts=[c[0] for c in counts],
                                                         seg_emb=embs[1], seg_counts=[c[1] for c in counts])
    torch.cuda.synchronize()
    assert torch.equal(kv[0][kv[1]:kv[1] + front], before), "the K / V front is read only"
    oc = os_ = 0
    for b, (nc, ns) in enumerate(counts):
        w_masks, w_cls, w_seg, _ = o.predictor_forward(desc, ms, shapes, prpos, mf, mf_size, seg_q[b * Q:(b + 1) * Q], class_emb=embs[0][oc:oc + nc],
                                                       seg_emb=embs[1][os_:os_ + ns], kv=kv)
        assert torch.equal(masks[b * Q:(b + 1) * Q], w_masks), b
        assert torch.equal(cls_l[Q * oc:Q * (oc + nc)].view(Q, nc), w_cls), b
        assert torch.equal(seg_l[Q * os_:Q * (os_ + ns)].view(Q, ns), w_seg), b
        oc, os_ = oc + nc, os_ + ns
    assert not torch.isnan(masks).any()


@pytest.mark.parametrize("size,B", [(384, 3), (640, 4)])                  # 640^2: the largest level has 6400 keys (100 chunks of 64)
def test_full_width_batched_stage_is_bitwise_the_per_prompt_loop(size, B):
    cfg, m = _model()
    mf_size, shapes = GEOM[size]
    _stage_vs_loop(cfg, m, mf_size, shapes, B, [(133, 1), (7, 1), (80, 1), (1, 1)][:B])


def test_full_width_segment_with_the_batched_decoder_is_bitwise_the_loop():
    cfg, m = _model()
    inp = fix_indices(session_inputs(cfg, "referring", 3))
    kw = {k: v for k, v in seg_kwargs(inp).items() if k != "is_thing_list"}
    sess = m.encode_image(inp["images"][:1], inp["seg_info"][0])
    res = {}
    try:
        for on in (False, True):
            m.batch_decoder = on
            res[on] = (m.segment(sess, postprocess=False, **kw), m.segment(sess, **seg_kwargs(inp)))
    finally:
        del m.batch_decoder
    torch.cuda.synchronize()
    for a, b in zip(res[True][0], res[False][0]):
        assert torch.equal(a["pred_masks"], b["pred_masks"]) and torch.equal(a["pred_SEG_logits"], b["pred_SEG_logits"])
    for a, b in zip(res[True][1], res[False][1]):
        assert torch.equal(a["mask_pred"], b["mask_pred"]) and torch.equal(a["instances"].scores, b["instances"].scores)
        assert torch.equal(a["instances"].pred_masks, b["instances"].pred_masks)


def test_mask_gemm_form_at_the_benchmark_geometries():
    """The split-f16 mask GEMM (B * Q, mask_dim) . mask_features^T picks its kernel form by M.  At mask_dim 256 (K = 3 * 256) psalm_gemm_describe
    reports the SAME form -- 64 x 128 tiles, un-split -- for M = Q = 100 and for every M = B * Q up to B = 16 at the 384^2, 640^2 and 1024^2
    geometries (asserted here: the loader-wave forms that follow M need Kp >= 512, split-K needs K >= 1024), so no shape with a differing form
    exists there and the case run is 640^2 with B = 8.  A shape where the forms DO differ is the next test's."""
    cfg, m = _model()
    o = m.ops
    Q, K = cfg.md_queries, 3 * 256
    for size, (mf_size, _) in GEOM.items():
        N = mf_size[0] * mf_size[1]
        one = o.gemm_describe(Q, N, K, x3=True)
        for B in range(2, 17):
            assert o.gemm_describe(B * Q, N, K, x3=True) == one, (size, B)
    mf_size, shapes = GEOM[640]
    _stage_vs_loop(cfg, m, mf_size, shapes, 8, [(3, 1)] * 8)


def test_mask_gemm_selected_by_q_where_the_forms_differ():
    """mask_dim 512 (Kp = 512), 128 x 128 mask features, 37 queries, 6 prompts: psalm_gemm_describe reports 64 x 128 tiles for M = 37 and a 128 x 128
    loader-wave form for M = 222 -- another K loop.  The batched stage selects by Q, so the words stay the per-prompt call's."""
    cfg, m = _model(md_hidden=64, md_heads=2, md_dim_ff=128, md_dec_layers=3, md_gn_groups=8, md_queries=37, md_mask_dim=512)
    o = m.ops
    mf_size, shapes, B = (128, 128), [(4, 4), (8, 8), (16, 16)], 6
    one, many = o.gemm_describe(37, 128 * 128, 3 * 512, x3=True), o.gemm_describe(B * 37, 128 * 128, 3 * 512, x3=True)
    assert tuple(one[:3]) != tuple(many[:3]), (one, many)
    _stage_vs_loop(cfg, m, mf_size, shapes, B, [(2, 1)] * B)
