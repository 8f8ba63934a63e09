"""The kernels under the batched mask decoder (psalm_predictor_forward_batched): B query sets against ONE K / V, the exact-fp32 skinny GEMM over
many row tiles, and the grouped form for the heads' ragged last products.  Each is held, word for word, against what the per-prompt decoder
launches for one prompt alone: psalm_mha_attention_f32 with B = 1 and psalm_gemm with float32 operands and <= 192 rows.  Nothing here reorders a
sum, so no comparison has a tolerance."""
import ctypes

import pytest
import torch

from ops_backend import ops  # noqa: F401
from psalm_amd import hip_ops as H

_CASES = {}


def _attention_case(B, heads, Lq, Lk):
    """row-strided q / k / v views; an all-masked flagged row in prompt 1 only; a row of the last prompt whose only visible keys lie in the last chunk"""
    key = (B, heads, Lq, Lk)
    if key not in _CASES:
        D = heads * 32
        g = torch.Generator().manual_seed(7 * Lq + Lk + B)
        q = torch.randn(B * Lq, D + 8, generator=g)
        kv = torch.randn(Lk, 2 * D + 4, generator=g)
        mask = torch.rand(B, Lq, Lk, generator=g) < 0.6
        mask[:, 1, 0] = False                                            # (row 1 is all-masked in prompt 1 ONLY)
        mask[1, 1, :] = True
        mask[B - 1, 2, : Lk - 3] = True
        mask[B - 1, 2, Lk - 3:] = False
        flags = mask.all(-1)
        assert flags[1, 1] and int(flags.sum()) == 1
        _CASES[key] = (q, kv, mask.to(torch.uint8), flags.to(torch.uint8))
    return _CASES[key]


def _shared_vs_single(ops, B, heads, Lq, Lk):
    """(shared-call output, its partial states, per-prompt outputs, per-prompt partial states, splits)"""
    D = heads * 32
    q, kv, mask, flags = _attention_case(B, heads, Lq, Lk)
    d = ops.device
    qd, kvd, md, fd = q.to(d), kv.to(d), mask.to(d), flags.to(d)
    ops.lib.psalm_mha_attention_f32_workspace.restype = ctypes.c_long
    one = ops.lib.psalm_mha_attention_f32_workspace(1, heads, Lq, Lk)
    nb = ops.mha_attention_f32_shared_workspace(B, heads, Lq, Lk)
    assert nb == B * one                                                 # B times the partial states of a B = 1 call: the same chunk
    splits = one // (heads * Lq * 36 * 4)
    ws = torch.zeros(max(nb, 1), dtype=torch.uint8, device=d)
    got = ops.mha_attention_f32_shared(qd[:, 8:8 + D], kvd[:, :D], kvd[:, D + 4:], B, Lq, Lk, heads, md, fd.view(-1), workspace=ws)
    want, wpart = [], []
    for b in range(B):
        w1 = torch.zeros(max(one, 1), dtype=torch.uint8, device=d)
        want.append(ops.mha_attention(qd[b * Lq:(b + 1) * Lq, 8:8 + D], kvd[:, :D], kvd[:, D + 4:], 1, Lq, Lk, heads, md[b:b + 1].contiguous(),
                                      fd[b].contiguous(), workspace=w1).cpu())
        wpart.append(w1.cpu())
    return got.cpu(), ws.cpu(), want, wpart, splits


def _states(buf, heads, splits, Lq, b=0):
    """the written floats [O (32) | m | l] of set b's partial states (the two pad floats of a 36-float state are never written)"""
    n = heads * splits * Lq * 36
    return buf.view(torch.float32)[b * n:(b + 1) * n].view(-1, 36)[:, :34]


@pytest.mark.parametrize("B,heads,Lq,Lk", [
    (3, 4, 37, 203),      # three tiles in a four-wavefront group (an empty wavefront); an odd B (a block with one live set); Lk % 4 != 0; 11-key last chunk
    (2, 8, 100, 1024),    # 16 chunks of 64 keys, the word-wise mask path
    (5, 8, 100, 4160),    # the B-dependent chunk of psalm_mha_attention_f32 (192) differs from the pinned one (64)
    (3, 4, 128, 700),     # eight tiles: blocks of 16 wavefronts
])
def test_shared_kv_attention_is_bitwise_the_single_prompt_call(ops, B, heads, Lq, Lk):
    if (B, Lk) == (5, 4160):
        # the trap this case exists for, read off the workspace sizes: a B = 5 call of psalm_mha_attention_f32 merges other chunks than a B = 1 call
        ops.lib.psalm_mha_attention_f32_workspace.restype = ctypes.c_long
        per = heads * Lq * 36 * 4
        s5, s1 = ops.lib.psalm_mha_attention_f32_workspace(5, heads, Lq, Lk) // (5 * per), ops.lib.psalm_mha_attention_f32_workspace(1, heads, Lq, Lk) // per
        assert (s5, s1) == (-(-Lk // 192), -(-Lk // 64))
        assert ops.mha_attention_f32_shared_workspace(5, heads, Lq, Lk) == 5 * s1 * per
    got, part, want, wpart, splits = _shared_vs_single(ops, B, heads, Lq, Lk)
    assert splits == -(-Lk // 64) and splits > 1
    for b in range(B):
        assert torch.equal(got[b * Lq:(b + 1) * Lq], want[b]), b
        assert torch.equal(_states(part, heads, splits, Lq, b), _states(wpart[b], heads, splits, Lq)), b
    assert not torch.isnan(got).any()
    assert (got[1 * Lq + 1] != 0).any()                                   # the flagged row attends every key (mask2former_transformer_decoder.py:647)


def test_shared_kv_attention_without_mask_and_single_chunk(ops):
    """no mask, Lk = 64: the direct normalised store, no workspace"""
    B, heads, Lq, Lk = 3, 4, 37, 64
    D = heads * 32
    q, kv, _, _ = _attention_case(B, heads, Lq, 203)
    d = ops.device
    qd, kvd = q.to(d), kv[:Lk].to(d)
    assert ops.mha_attention_f32_shared_workspace(B, heads, Lq, Lk) == 0
    got = ops.mha_attention_f32_shared(qd[:, 8:8 + D], kvd[:, :D], kvd[:, D + 4:], B, Lq, Lk, heads).cpu()
    for b in range(B):
        want = ops.mha_attention(qd[b * Lq:(b + 1) * Lq, 8:8 + D], kvd[:, :D], kvd[:, D + 4:], 1, Lq, Lk, heads).cpu()
        assert torch.equal(got[b * Lq:(b + 1) * Lq], want)


def test_shared_kv_attention_both_kernel_forms(ops):
    """PSALM_TUNE_MHA_QTILE_WAVES on (two sets per block, a wavefront per query tile) and off (one wavefront per set): the same words, and each the
    single-prompt call's under the same setting"""
    B, heads, Lq, Lk = 3, 4, 37, 203
    res = {}
    try:
        for v in (1, 0):
            ops.set_tuning(ops.TUNE_MHA_QTILE_WAVES, v)
            got, part, want, wpart, splits = _shared_vs_single(ops, B, heads, Lq, Lk)
            for b in range(B):
                assert torch.equal(got[b * Lq:(b + 1) * Lq], want[b]), (v, b)
                assert torch.equal(_states(part, heads, splits, Lq, b), _states(wpart[b], heads, splits, Lq)), (v, b)
            res[v] = got
    finally:
        ops.set_tuning(ops.TUNE_MHA_QTILE_WAVES, 1)
    assert torch.equal(res[0], res[1])


# ---------------------------------------------------------------------------------------------------------------- skinny GEMM over many row tiles
def _rows_case(B, Q, N, K):
    key = ("rows", B, Q, N, K)
    if key not in _CASES:
        g = torch.Generator().manual_seed(B * Q + N + K)
        _CASES[key] = (torch.randn(B * Q, K + 4, generator=g), torch.randn(N, K, generator=g), torch.randn(N, generator=g),
                       torch.randn(B * Q, N + 4, generator=g))
    return _CASES[key]


@pytest.mark.parametrize("B,Q", [(3, 37), (5, 100)])                      # M = 111 / 500 (above psalm_gemm's 192), 32-row tile boundaries inside prompts
@pytest.mark.parametrize("N", [256, 72])
@pytest.mark.parametrize("K", [64, 256])                                  # 4 / 16 wavefronts split K
def test_gemm_f32_rows_is_bitwise_the_per_prompt_gemm(ops, B, Q, N, K):
    a, w, bias, res = _rows_case(B, Q, N, K)
    d = ops.device
    ad, wd, bd, rd = a.to(d)[:, :K], w.to(d), bias.to(d), res.to(d)[:, :N]       # (row-strided A / residual views)
    forms = [dict(), dict(bias=bd, act=H.ACT_RELU), dict(bias=bd, residual=rd), dict(residual=rd)]
    for kw in forms:
        got = ops.gemm_f32_rows(ad, wd, **kw).cpu()
        assert ops.lib.psalm_gemm_last_kernel().decode() == f"gemm_f32_skinny_kernel<float, {16 if K >= 256 else 4}>"
        for b in range(B):
            kb = dict(kw)
            if "residual" in kb:
                kb["residual"] = rd[b * Q:(b + 1) * Q]
            want = ops.gemm(ad[b * Q:(b + 1) * Q], wd, **kb).cpu()
            assert ops.lib.psalm_gemm_last_kernel().decode() == f"gemm_f32_skinny_kernel<float, {16 if K >= 256 else 4}>"
            assert torch.equal(got[b * Q:(b + 1) * Q], want), (sorted(kw), b)


@pytest.mark.parametrize("B,Q", [(3, 37), (5, 100)])
@pytest.mark.parametrize("K", [64, 256])
def test_gemm_f32_rows_pair_is_bitwise_the_per_prompt_gemm(ops, B, Q, K):
    a0, w0, b0, _ = _rows_case(B, Q, 256, K)
    a1, w1, b1, _ = _rows_case(B, Q, 72, K)
    d = ops.device
    a0d, a1d = a0[:, :K].contiguous().to(d), (a1[:, :K] * 0.5).contiguous().to(d)
    w0d, w1d, b0d, b1d = w0.to(d), w1.to(d), b0.to(d), b1.to(d)
    c0, c1 = ops.gemm_f32_rows_pair(a0d, w0d, b0d, a1d, w1d, None, act0=H.ACT_RELU)
    c0, c1 = c0.cpu(), c1.cpu()
    for b in range(B):
        s = slice(b * Q, (b + 1) * Q)
        assert torch.equal(c0[s], ops.gemm(a0d[s], w0d, b0d, act=H.ACT_RELU).cpu()), b
        assert torch.equal(c1[s], ops.gemm(a1d[s], w1d).cpu()), b
    if B * Q > 192:
        with pytest.raises(H.PsalmHipError, match="psalm_gemm_f32_pair: M <= 192"):
            ops.gemm_f32_pair(a0d, w0d, b0d, a1d, w1d, None)             # the per-prompt entry keeps its range


def test_gemm_f32_rows_limits(ops):
    d = ops.device
    with pytest.raises(H.PsalmHipError, match="psalm_gemm_f32_rows: M <= 2048"):
        ops.gemm_f32_rows(torch.zeros(2049, 8, device=d), torch.zeros(8, 8, device=d))
    with pytest.raises(H.PsalmHipError, match="psalm_gemm_f32_rows: M <= 2048"):
        ops.gemm_f32_rows(torch.zeros(8, 12, device=d), torch.zeros(8, 12, device=d))            # K % 8


# ---------------------------------------------------------------------------------------------------------------- grouped head products
@pytest.mark.parametrize("Q,K", [(37, 64), (100, 256)])
def test_gemm_f32_grouped_is_bitwise_the_per_prompt_gemm(ops, Q, K):
    """counts {5, 1, 9}: class-shaped problems (Q, n_b) = h_b . emb_b^T and region-shaped ones (n_b, Q) = emb_b . h_b^T, each one launch"""
    counts = [5, 1, 9]
    g = torch.Generator().manual_seed(Q + K)
    d = ops.device
    h = torch.randn(len(counts) * Q, K, generator=g).to(d)
    emb = torch.randn(sum(counts), K, generator=g).to(d)
    hs = [h[b * Q:(b + 1) * Q] for b in range(len(counts))]
    es, o = [], 0
    for n in counts:
        es.append(emb[o:o + n])
        o += n
    for A, W in ((hs, es), (es, hs)):
        got = ops.gemm_f32_grouped(A, W)
        assert ops.lib.psalm_gemm_last_kernel().decode() == f"gemm_f32_skinny_group_kernel<float, {16 if K >= 256 else 4}>"
        for b, (a_, w_) in enumerate(zip(A, W)):
            assert tuple(got[b].shape) == (a_.shape[0], w_.shape[0])
            assert torch.equal(got[b].cpu(), ops.gemm(a_, w_).cpu()), b


def test_gemm_f32_grouped_skips_empty_problems_and_checks_its_range(ops):
    d = ops.device
    g = torch.Generator().manual_seed(3)
    h = torch.randn(37, 64, generator=g).to(d)
    e = torch.randn(4, 64, generator=g).to(d)
    got = ops.gemm_f32_grouped([h, h], [e[:0], e])
    assert tuple(got[0].shape) == (37, 0) and torch.equal(got[1].cpu(), ops.gemm(h, e).cpu())
    with pytest.raises(H.PsalmHipError, match="psalm_gemm_f32_grouped: M <= 192"):
        ops.gemm_f32_grouped([torch.zeros(193, 64, device=d)], [e])
    with pytest.raises(H.PsalmHipError, match="1..16 problems"):
        ops.gemm_f32_grouped([h] * 17, [e] * 17)
