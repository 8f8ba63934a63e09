"""The mask decoder's serial tail: the query-tile-parallel form of psalm_mha_attention_f32 (PSALM_TUNE_MHA_QTILE_WAVES: a wavefront per 16-query
tile instead of one wavefront that walks all tiles), the further psalm_gemm_f32_pair launches of psalm_predictor_forward (PSALM_TUNE_DECODER_FUSE)
and the stage results written where they are wanted (no final device copies).  All of it reorders launches or work between wavefronts and none of
it reorders a sum: every comparison here is word for word."""
import dataclasses

import pytest
import torch

from ops_backend import ops  # noqa: F401
from psalm_amd.config import PsalmConfig
from psalm_amd.model import PSALM
from psalm_amd.synthetic import make_state_dict


def _attention_case(B, heads, Lq, Lk, masked):
    """operands as in test_mha_attention_f32_matrix_core_split_kv: row-strided views; an all-masked flagged row and a row whose only visible
    keys lie in the last chunk"""
    hd = 32
    D = heads * hd
    g = torch.Generator().manual_seed(Lq + Lk)
    q = torch.randn(B * Lq, D + 8, generator=g)
    kv = torch.randn(B * Lk, 2 * D + 4, generator=g)
    mask = flags = None
    if masked:
        mask = torch.rand(B, Lq, Lk, generator=g) < 0.6
        mask[0, 1, :] = True
        mask[B - 1, 2, : Lk - 3] = True
        flags = mask.all(-1)
    return q, kv, mask, flags


def _attention_want(q, kv, mask, flags, B, heads, Lq, Lk):
    hd = 32
    D = heads * hd
    qq, kk, vv = q[:, 8:8 + D], kv[:, :D], kv[:, D + 4:]
    a = (qq.view(B, Lq, heads, hd).transpose(1, 2) * hd ** -0.5) @ kk.reshape(B, Lk, heads, hd).transpose(1, 2).transpose(-2, -1)
    if mask is not None:
        wm = mask.clone()
        wm[flags] = False
        a = a.masked_fill(wm[:, None], float("-inf"))
    return (a.softmax(-1) @ vv.reshape(B, Lk, heads, hd).transpose(1, 2)).transpose(1, 2).reshape(B * Lq, D)


@pytest.mark.parametrize("B,heads,Lq,Lk,masked,vs_torch", [
    (2, 4, 12, 64, True, False),          # one tile, one chunk: the direct normalised store
    (2, 4, 37, 203, True, False),         # three tiles in the four-wavefront block (an empty wavefront); Lk % 4 != 0: the slow mask path; 11-key last chunk
    (2, 4, 100, 100, False, False),       # the self-attention shape: seven tiles, the last with 4 rows; chunks of 64 and 36 keys
    (1, 8, 100, 1024, True, False),       # 16 chunks of 64 keys, the word-wise mask path
    (2, 4, 128, 700, True, False),        # eight tiles
    (2, 8, 100, 4160, True, True),        # 128-key chunks: two LDS tiles per chunk (the double buffer); the last chunk has 64 keys
])
def test_mha_attention_f32_query_tile_waves_are_bitwise_the_one_wave_kernel(ops, B, heads, Lq, Lk, masked, vs_torch):
    """Each query tile's values are touched only by its own instructions, in key order, so giving every tile a wavefront of its own returns the
    words of the one-wave kernel: the output (after the combine where the keys are split) and the partial states in the workspace.  The last
    case is also held against torch fp32 at test_mha_attention_f32_matrix_core_split_kv's tolerance."""
    D = heads * 32
    q, kv, mask, flags = _attention_case(B, heads, Lq, Lk, masked)
    d = ops.device
    qd, kvd = q.to(d), kv.to(d)
    md = mask.to(torch.uint8).to(d) if masked else None
    fd = flags.to(torch.uint8).to(d) if masked else None
    ops.lib.psalm_mha_attention_f32_workspace.restype = __import__("ctypes").c_long
    nbytes = ops.lib.psalm_mha_attention_f32_workspace(B, heads, Lq, Lk)
    assert (nbytes > 0) == (Lk > 64)
    got, part = {}, {}
    try:
        for v in (0, 1):
            ops.set_tuning(ops.TUNE_MHA_QTILE_WAVES, v)
            got[v] = ops.mha_attention(qd[:, 8:8 + D], kvd[:, :D], kvd[:, D + 4:], B, Lq, Lk, heads, md, fd).cpu()
            if nbytes:
                part[v] = ops._ws[("mha_f32_ws", nbytes)].cpu().clone()
    finally:
        ops.set_tuning(ops.TUNE_MHA_QTILE_WAVES, 1)
    assert torch.equal(got[0], got[1])
    if nbytes:
        assert torch.equal(part[0], part[1])
    if vs_torch:
        want = _attention_want(q, kv, mask, flags, B, heads, Lq, Lk)
        assert (got[1] - want).abs().max() <= 2e-5 * want.abs().max()


def test_mha_qtile_waves_is_the_default(ops):
    assert ops.get_tuning(ops.TUNE_MHA_QTILE_WAVES) == 1


def _tiny_model(ops, queries=37):                                                  # 37: three query tiles, the last with 5 rows
    cfg = dataclasses.replace(PsalmConfig.tiny("panoptic"), md_queries=queries)
    sd = make_state_dict(cfg, seed=11)
    m = PSALM(cfg, sd, ops=ops, precision="f16x3")
    assert m.c_stages
    return cfg, m


def _both_settings(ops, fn):
    """fn() with (query-tile waves, decoder pairs) on and with both off"""
    outs = []
    try:
        for v in (1, 0):
            ops.set_tuning(ops.TUNE_MHA_QTILE_WAVES, v)
            ops.set_tuning(ops.TUNE_DECODER_FUSE, v)
            outs.append(fn())
    finally:
        ops.set_tuning(ops.TUNE_MHA_QTILE_WAVES, 1)
        ops.set_tuning(ops.TUNE_DECODER_FUSE, 1)
    return outs


def test_pixel_decoder_stage_writes_its_level_tokens_in_place(ops):
    """psalm_pixel_decoder_forward: the last encoder layer's norm2 writes the level tokens into the result buffer (it was a device copy at the end),
    and the FPN step reads its level from there.  Held against the op-by-op sequence, word for word."""
    cfg, m = _tiny_model(ops)
    g = torch.Generator().manual_seed(5)
    dims = [cfg.swin_embed_dim * 2 ** i for i in range(4)]
    feats = [(torch.randn(h * w, c, generator=g).to(ops.device), h, w) for c, (h, w) in zip(dims, ((16, 12), (8, 6), (4, 3), (2, 2)))]

    def run():
        mf, ms, _, _ = m.pixel_decoder(feats)
        return [mf.cpu().clone()] + [t.cpu().clone() for t in ms]

    new, old = _both_settings(ops, run)
    assert ("pd_desc",) in m._cache
    m.c_stages = False
    ref = run()
    assert len(new) == len(old) == len(ref) == 4
    for a, b, c in zip(new, old, ref):
        assert torch.equal(a, b) and torch.equal(a, c)


@pytest.mark.parametrize("heads_wanted,mf_size,queries", [
    (("class", "seg"), (24, 20), 37),
    (("class", "region"), (24, 20), 37),          # a pair of embedding products with different row counts
    (("class", "seg", "region"), (24, 20), 37),   # two heads paired, the third on its own
    (("seg",), (24, 20), 37),
    (("class", "seg"), (68, 64), 12),             # > 4096 pixels: the mask GEMM in split-f16 arithmetic
])
def test_predictor_stage_pairs_and_in_place_masks_are_bitwise(ops, heads_wanted, mf_size, queries):
    """psalm_predictor_forward with (query-tile waves, more GEMM pairs) and with (the one-wave kernel, the r05 launch sequence): pred_masks -- written by
    the last mask head itself -- and every requested head's logits, word for word; and both against the op-by-op sequence."""
    cfg, m = _tiny_model(ops, queries)
    D, Q, MD = cfg.md_hidden, cfg.md_queries, cfg.md_mask_dim
    g = torch.Generator().manual_seed(7)
    d = ops.device
    shapes = [(3, 3), (6, 5), (12, 10)]
    ms = [torch.randn(h * w, D, generator=g).to(d) for h, w in shapes]
    mf = torch.randn(mf_size[0] * mf_size[1], MD, generator=g).to(d)
    seg_query = torch.randn(Q, D, generator=g).to(d)
    emb = {"class_emb": torch.randn(10, D, generator=g).to(d) if "class" in heads_wanted else None,
           "SEG_emb": torch.randn(1, D, generator=g).to(d) if "seg" in heads_wanted else None,
           "region_emb": torch.randn(5, D, generator=g).to(d) if "region" in heads_wanted else None}
    keys = ("pred_masks", "pred_class_name_logits", "pred_SEG_logits", "pred_region_logits")

    def run():
        r = m.predictor(ms, shapes, mf, mf_size, seg_query, **emb)
        return {k: (None if r[k] is None else r[k].cpu().clone()) for k in keys}

    new, old = _both_settings(ops, run)
    assert ("pr_desc",) in m._cache
    m.c_stages = False
    ref = run()
    for k, want in (("pred_class_name_logits", "class"), ("pred_SEG_logits", "seg"), ("pred_region_logits", "region")):
        assert (new[k] is not None) == (want in heads_wanted)
    for k in keys:
        for other in (old, ref):
            assert (new[k] is None) == (other[k] is None) and (new[k] is None or torch.equal(new[k], other[k])), k
