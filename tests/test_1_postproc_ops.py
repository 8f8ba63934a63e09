"""Op-level tests of the post-processing kernels that were reached only through whole-model runs, where a wrong edge is one pixel or one query
among thousands: psalm_class_softmax, psalm_sigmoid_transpose, psalm_binarize_gather, psalm_region_scores, psalm_region_pool, psalm_mask_scores
(+ the mask-score output of both fused semantic passes) at their edges, and psalm_panoptic on either side of the Q = 128 switch between its two
merge kernels.  Every reference is float64 torch or exact integer logic.  Runs on the host emulation of the kernels here and on the real GPU
under `-m gpu`."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from ops_backend import ops  # noqa: F401
from oracle import psalm_oracle as O


# ------------------------------------------------------------------------------------------------ class softmax
_CLS = {}


def _class_case(Q, C1):
    """logits randn * 8 with planted rows: exact ties of the maximum in two lanes of the wavefront (columns c, c + 64: the same lane; c, c + 1:
    neighbouring lanes; c, c + 3 further apart), and a row whose maximum is the void column"""
    if (Q, C1) not in _CLS:
        g = torch.Generator().manual_seed(Q * 1000 + C1)
        cls = torch.randn(Q, C1, generator=g) * 8
        top = cls.abs().max() + 3
        planted = {}
        if C1 > 64 + 2:
            cls[0, [2, 2 + 64]] = top                               # same lane (one lane walks c, c + 64, ...): the earlier one wins
            planted[0] = 2
            cls[4 % Q, [C1 - 1 - 64, C1 - 1]] = top                 # ... the later one being the void column
            planted[4 % Q] = C1 - 1 - 64
        cls[1, [5, 6]] = top                                        # neighbouring lanes
        planted[1] = 5
        cls[2, [C1 - 2, 1]] = top                                   # far apart, written in the other order
        planted[2] = 1
        cls[3, C1 - 1] = top                                        # the void column is the maximum
        planted[3] = C1 - 1
        _CLS[(Q, C1)] = (cls, planted)
    return _CLS[(Q, C1)]


@pytest.mark.parametrize("tdtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("Q,C1", [(100, 134), (7, 10), (5, 65), (129, 460)])
def test_class_softmax(ops, Q, C1, tdtype):
    cls, planted = _class_case(Q, C1)
    want = cls.double().softmax(-1)
    wmax, widx = torch.max(cls, 1)                                  # first index on ties
    for q, cidx in planted.items():
        assert widx[q] == cidx
    for Kpad in sorted({(Q + 63) // 64 * 64, (Q + 127) // 128 * 128}):
        probs, probsT, score, label = ops.class_softmax(cls.to(ops.device), Kpad, probsT_dtype=tdtype)
        probs, probsT, score, label = probs.cpu(), probsT.cpu(), score.cpu(), label.cpu()
        assert torch.equal(label.long(), widx)
        assert torch.equal(score, probs.max(1).values)              # bit for bit
        err = (probs.double() - want).abs().max()
        print(f"class_softmax ({Q}, {C1}): max err {err:.3e}")
        assert err <= 3e-6
        assert probsT.shape == (C1 - 1, Kpad) and probsT.dtype == tdtype
        assert torch.equal(probsT[:, :Q], probs[:, :-1].T.to(tdtype))
        assert (probsT[:, Q:] == 0).all()


# ------------------------------------------------------------------------------------------------ sigmoid + transpose
@pytest.mark.parametrize("odtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("Q,HW,Kpad", [(100, 64 * 3 + 40, 128), (12, 50, 64), (70, 64, 128)])
def test_sigmoid_transpose(ops, Q, HW, Kpad, odtype):
    g = torch.Generator().manual_seed(Q + HW)
    mask = torch.randn(Q, HW, generator=g) * 6
    mask[0, :4] = torch.tensor([0.0, -0.0, 40.0, -40.0])
    got = ops.sigmoid_transpose(mask.to(ops.device), Kpad, odtype).cpu()
    want = mask.double().sigmoid().T
    assert got.shape == (HW, Kpad) and got.dtype == odtype
    # fp32: the device exp / reciprocal are good to a few ulp (values in [0, 1]: 4 ulp of 1); bf16: its unit roundoff 2^-8 (8 significand bits,
    # round to nearest) of the value on top of that
    tol = 4 * 2.0 ** -23 if odtype == torch.float32 else 2.0 ** -8 * want + 4 * 2.0 ** -23
    assert ((got[:, :Q].double() - want).abs() <= tol).all()
    assert (got[:, Q:] == 0).all()


# ------------------------------------------------------------------------------------------------ binarize + gather
def _binarize(ops, mask, out, query, count):
    """the C entry point as Ops.binarize_gather calls it, into a buffer the test owns"""
    n, HW = out.shape[0], mask.shape[1] * mask.shape[2]
    rc = ops.lib.psalm_binarize_gather(ops._p(mask), ops._p(query), ops._p(count), ops._p(out), n, ctypes.c_long(HW), ops._stream())
    ops._check(rc, "psalm_binarize_gather")


@pytest.mark.parametrize("HW", [1, 1023, 1024 * 3 + 5])
def test_binarize_gather(ops, HW):
    d = ops.device
    Q = 6
    g = torch.Generator().manual_seed(HW)
    mask = torch.randn(Q, 1, HW, generator=g)
    edge = torch.tensor([0.0, -0.0, 1e-45, -1e-45, 1.17549435e-38])          # the rule is > 0: zeros no, a denormal yes
    for q in range(Q):
        mask[q, 0, : min(HW, 5)] = edge.roll(q)[: min(HW, 5)]
    want_all = (mask.double() > 0).float()
    assert want_all[:, 0, 0].tolist() == [float(v > 0) for v in [0.0, 1.17549435e-38, -1e-45, 1e-45, -0.0, 0.0]]
    # without query / count: every row in place
    out = ops.empty(Q, 1, HW)
    out.fill_(-7.0)
    _binarize(ops, mask.to(d), out, None, None)
    assert torch.equal(out.cpu(), want_all)
    assert torch.equal(ops.binarize_gather(mask.to(d), Q).cpu(), want_all)
    # a query list that repeats an index, count < n: rows >= count untouched
    n = 5
    query = torch.tensor([3, 0, 3, 5, 1], dtype=torch.int32)
    count = torch.tensor([3], dtype=torch.int32)
    out = ops.empty(n, 1, HW)
    out.fill_(-7.0)
    _binarize(ops, mask.to(d), out, query.to(d), count.to(d))
    out = out.cpu()
    assert torch.equal(out[:3], want_all[query[:3].long()])
    assert (out[3:] == -7.0).all()


# ------------------------------------------------------------------------------------------------ region scores
@pytest.mark.parametrize("K,Q", [(1, 100), (7, 100), (33, 12)])
def test_region_scores(ops, K, Q):
    g = torch.Generator().manual_seed(K + Q)
    logits = torch.randn(K, Q, generator=g) * 5
    ms = torch.rand(Q, generator=g)
    ms[0] = 0.0
    got = ops.region_scores(logits.to(ops.device), ms.to(ops.device)).cpu()
    want = logits.double().sigmoid().T * ms.double()[:, None]
    assert got.shape == (Q, K)
    assert (got.double() - want).abs().max() <= 4 * 2.0 ** -23      # values in [0, 1]: a few ulp of 1 for the device exp / reciprocal
    assert (got[0] == 0).all()


# ------------------------------------------------------------------------------------------------ region pooling
@pytest.mark.parametrize("h,w", [(1, 1), (5, 7), (24, 24)])
@pytest.mark.parametrize("n", [1, 256])
@pytest.mark.parametrize("C", [40, 256, 300])
def test_region_pool(ops, C, n, h, w):
    """grid_sample(align_corners=True, zero padding) + the mean over the points: oracle/psalm_oracle.py: region_pooling (CC:333-400)"""
    g = torch.Generator().manual_seed(C + n + h * w)
    n_img = 2
    tokens = torch.randn(n_img * h * w, C, generator=g)
    img = torch.tensor([1, 0, 1, 1, 0], dtype=torch.int32)          # regions addressed out of order
    R = img.numel()
    pts = torch.rand(R, n, 2, generator=g)
    one_m = 1.0 - 2.0 ** -24
    edge = torch.tensor([[0.0, 0.0], [1.0, 1.0], [one_m, one_m], [0.0, 1.0], [1.0, 0.0], [one_m, 0.5], [0.5, 1.0]])
    if h > 1 and w > 1:
        edge = torch.cat((edge, torch.tensor([[2.0 / (h - 1), 3.0 / (w - 1)], [1.0 / (h - 1), 1.0]])))    # exactly on a grid node
    for r in range(R):
        if n == 1:
            pts[r, 0] = edge[r % edge.shape[0]]
        else:
            pts[r, : edge.shape[0]] = edge.roll(r, 0)
    got = ops.region_pool(tokens.to(ops.device), img.to(ops.device), pts.to(ops.device), h, w, n_img).cpu()
    fmap = tokens.double().view(n_img, h, w, C).permute(0, 3, 1, 2)[img.long()]              # (R, C, h, w)
    grid = (2.0 * pts.double().flip(dims=(2,)) - 1.0).unsqueeze(2)                           # (x, y)
    want = F.grid_sample(fmap, grid, align_corners=True, padding_mode="zeros").squeeze(3).mean(-1)
    assert got.shape == (R, C) and torch.isfinite(got).all()
    assert (got.double() - want).abs().max() <= 1e-5 * want.abs().max()


# ------------------------------------------------------------------------------------------------ mask scores
@pytest.mark.parametrize("Q,HW", [(5, 1), (7, 40), (12, 63), (100, 300)])
def test_mask_scores_edges(ops, Q, HW):
    """HW < 64: some of the 64 chunks of the partial kernel are empty; a query with no positive pixel scores exactly 0; a query with one"""
    g = torch.Generator().manual_seed(Q * HW)
    mask = torch.randn(Q, HW, generator=g) * 4
    mask[0] = -mask[0].abs()                                        # all <= 0 ...
    mask[0, 0] = 0.0                                                # ... a zero included
    mask[1] = -mask[1].abs() - 0.1
    mask[1, HW - 1] = 2.5                                           # a single positive pixel, the last one
    pos = (mask > 0).double()
    want = (mask.double().sigmoid() * pos).sum(1) / (pos.sum(1) + 1e-6)                      # LP:443-444
    d = ops.device
    got = ops.mask_scores(mask.to(d)).cpu()
    assert got[0] == 0
    assert (got.double() - want).abs().max() < 1e-5
    C = 9
    cls = torch.randn(Q, C + 1, generator=g)
    for dt in (torch.bfloat16, torch.float32):                      # the fused semantic passes accumulate the score from the same read
        probsT = ops.class_softmax(cls.to(d), 128, probsT_dtype=dt)[1]
        sem, ms = ops.semantic_from_masks(mask.to(d), probsT, want_mask_score=True)
        ms = ms.cpu()
        assert ms[0] == 0
        assert (ms.double() - want).abs().max() < 1e-5
        full = torch.einsum("qc,qp->cp", cls.double().softmax(-1)[:, :-1], mask.double().sigmoid())
        assert (sem.cpu().double() - full).abs().max() <= (2 ** -7 if dt == torch.bfloat16 else 4e-6) * full.abs().max() + 1e-7


# ------------------------------------------------------------------------------------------------ panoptic, both merge kernels
_PAN = {}


def _panoptic_inputs(Q, C, Hh, Ww):
    """the blob construction of tests/test_1_ops.py::test_panoptic_matches_oracle_inference"""
    if (Q, C, Hh, Ww) not in _PAN:
        g = torch.Generator().manual_seed(Q + Hh * Ww)
        yy, xx = torch.meshgrid(torch.arange(Hh), torch.arange(Ww), indexing="ij")
        mask = torch.randn(Q, Hh, Ww, generator=g) * 0.7 - 5.0
        for q in range(Q):
            if q % 3 == 2:
                continue
            cy, cx = int(torch.randint(0, Hh, (1,), generator=g)), int(torch.randint(0, Ww, (1,), generator=g))
            r = int(torch.randint(1, max(2, min(Hh, Ww) // 12), (1,), generator=g))
            mask[q][((yy - cy).abs() <= r) & ((xx - cx).abs() <= r)] += 9.0
        mask[:, 0, :3] = 0.0
        cls = torch.randn(Q, C + 1, generator=g)
        hot = torch.randint(0, C + 1, (Q,), generator=g)
        cls[torch.arange(Q), hot] += torch.where(torch.rand(Q, generator=g) < 0.7, 8.0, 1.0)
        thing = [int(v) for v in (torch.rand(C, generator=g) < 0.6)]
        _PAN[(Q, C, Hh, Ww)] = (mask, cls, thing)
    return _PAN[(Q, C, Hh, Ww)]


@pytest.mark.parametrize("Qfull,C,Hh,Ww", [(129, 20, 64, 64), (200, 20, 61, 67)])        # (few classes: several kept queries share a stuff class)
def test_panoptic_above_and_below_the_merge_switch(ops, Qfull, C, Hh, Ww):
    """Q > 128 takes the one-thread panoptic_merge_kernel, Q <= 128 the one-thread-per-query panoptic_merge_par_kernel: the same inputs, whole and
    truncated to 128 queries, each against the oracle's restatement of class_name_panoptic_inference -- identical id map and segments_info."""
    mask, cls, thing = _panoptic_inputs(Qfull, C, Hh, Ww)
    d = ops.device
    for Q in (Qfull, 128):
        m, c = mask[:Q].contiguous(), cls[:Q].contiguous()
        want_pan, want_info = O.panoptic_inference(c, m, thing)
        probs, probsT, score, label = ops.class_softmax(c.to(d), (Q + 63) // 64 * 64)
        pan, info, ninfo = ops.panoptic(m.to(d), score, label, torch.tensor(thing, dtype=torch.int32, device=d), C, 0.8, 0.8)
        n = int(ninfo.item())
        got_info = [{"id": a, "isthing": bool(b), "category_id": c_} for a, b, c_ in info.cpu()[:n].tolist()]
        assert len(want_info) >= 8                                  # the case exercises the merge ...
        stuff = [s["category_id"] for s in want_info if not s["isthing"]]
        kept_stuff = sum(1 for q in range(Q) if float(probs[q].max()) > 0.8 and int(label[q]) != C and not thing[int(label[q])])
        assert kept_stuff > len(stuff)                              # ... and queries join an open stuff segment
        assert got_info == want_info
        assert torch.equal(pan.cpu(), want_pan)
