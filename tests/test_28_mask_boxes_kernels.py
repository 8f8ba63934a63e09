"""psalm_mask_boxes / psalm_label_boxes (csrc/maskbox.hip) against numpy on the very same masks: detectron2's BitMasks.get_bounding_boxes
convention, (x_min, y_min, x_max + 1, y_max + 1) over the set pixels, zeros for an empty mask, area = set pixels.  Integer results: every
comparison is exact.  Runs on the host emulation of the kernel sources and, marked gpu, on the MI355X."""
import numpy as np
import pytest
import torch

from ops_backend import ops  # noqa: F401  (fixture)
from psalm_amd.hip_ops import PsalmHipError


def np_boxes(masks, fp32):
    """the oracle: set = (f > 0) for float32, (!= 0) for bytes"""
    boxes, areas = np.zeros((len(masks), 4), np.float32), np.zeros(len(masks), np.int32)
    for i, m in enumerate(masks):
        with np.errstate(invalid="ignore"):
            ys, xs = np.nonzero(m > 0 if fp32 else m != 0)
        if len(ys):
            boxes[i] = [xs.min(), ys.min(), xs.max() + 1, ys.max() + 1]
        areas[i] = len(ys)
    return boxes, areas


def check(ops, masks_np, dtype, index=None):
    fp32 = dtype == torch.float32
    t = torch.from_numpy(masks_np).to(ops.device)
    t = t.to(dtype) if dtype != torch.bool else t != 0
    idx = None if index is None else torch.tensor(index, dtype=torch.int32, device=ops.device)
    boxes, areas = ops.mask_boxes(t, index=idx)
    want_b, want_a = np_boxes(masks_np, fp32)
    if index is not None:
        n = len(masks_np)
        sel = [i if 0 <= i < n else None for i in index]
        want_b = np.stack([want_b[i] if i is not None else np.zeros(4, np.float32) for i in sel])
        want_a = np.array([want_a[i] if i is not None else 0 for i in sel], np.int32)
    assert boxes.dtype == torch.float32 and areas.dtype == torch.int32 and boxes.device == t.device
    assert tuple(boxes.shape) == (len(want_a), 4) and tuple(areas.shape) == (len(want_a),)
    assert np.array_equal(boxes.cpu().numpy(), want_b), (boxes.cpu().numpy(), want_b)
    assert np.array_equal(areas.cpu().numpy(), want_a), (areas.cpu().numpy(), want_a)
    return boxes, areas


def blobs(n, H, W, seed):
    """random rectangles and discs, several per plane, of values 1..3"""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W]
    out = np.zeros((n, H, W), np.uint8)
    for i in range(n):
        for _ in range(3):
            cy, cx, r = g.integers(0, H), g.integers(0, W), g.integers(3, max(4, min(H, W) // 3))
            if g.integers(2):
                out[i][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = g.integers(1, 4)
            else:
                out[i, max(0, cy - r): cy + r, max(0, cx - 2 * r): cx + 2 * r] = g.integers(1, 4)
    return out


DTYPES = [torch.float32, torch.uint8]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "u8"])
@pytest.mark.parametrize("corner", [(0, 0), (0, 149), (69, 0), (69, 149)], ids=["tl", "tr", "bl", "br"])
def test_shapes_70x150(ops, dtype, corner):
    """(6, 70, 150): W no multiple of 64 and wider than two ballot words; empty, full, one corner pixel, a full row, a full column, two pixels
    astride the 64-element boundary"""
    m = np.zeros((6, 70, 150), np.uint8)
    m[1] = 1
    m[2][corner] = 1
    m[3, 41, :] = 1
    m[4, :, 77] = 1
    m[5, 33, 63] = m[5, 34, 64] = 1
    boxes, areas = check(ops, m, dtype)
    assert areas.tolist() == [0, 70 * 150, 1, 150, 70, 2]
    assert boxes[5].tolist() == [63, 33, 65, 35] and boxes[0].tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("dtype", DTYPES + [torch.bool], ids=["f32", "u8", "bool"])
def test_misaligned_planes(ops, dtype):
    """(5, 33, 67): odd W, H * W = 2211 no multiple of 4, so every plane after the first (and every row after the first) starts misaligned; a
    storage offset of one element shifts plane 0 as well"""
    m = blobs(5, 33, 67, 1)
    m[3] = 0
    m[3, 32, 66] = 2
    m[4] = 0
    m[4, 0, 0] = m[4, 17, 3] = 1
    check(ops, m, dtype)
    flat = torch.zeros(5 * 33 * 67 + 1, dtype=torch.float32 if dtype == torch.float32 else torch.uint8, device=ops.device)
    flat[1:] = torch.from_numpy(m.reshape(-1)).to(ops.device).to(flat.dtype)
    shifted = flat[1:].view(5, 33, 67)
    boxes, areas = ops.mask_boxes(shifted)
    wb, wa = np_boxes(m, dtype == torch.float32)
    assert np.array_equal(boxes.cpu().numpy(), wb) and np.array_equal(areas.cpu().numpy(), wa)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "u8"])
def test_blobs_several_blocks(ops, dtype):
    """(2, 200, 600): random blobs over several row groups (blocks) and several steps of a row; called twice: the same bytes (integer atomics)"""
    m = blobs(2, 200, 600, 2)
    b1, a1 = check(ops, m, dtype)
    b2, a2 = check(ops, m, dtype)
    assert b1.cpu().numpy().tobytes() == b2.cpu().numpy().tobytes() and a1.cpu().numpy().tobytes() == a2.cpu().numpy().tobytes()
    assert (a1 > 0).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "u8"])
def test_single_pixel_and_none(ops, dtype):
    check(ops, np.ones((1, 1, 1), np.uint8), dtype)
    check(ops, np.zeros((1, 1, 1), np.uint8), dtype)
    boxes, areas = ops.mask_boxes(torch.zeros(0, 7, 9, dtype=dtype, device=ops.device))
    assert tuple(boxes.shape) == (0, 4) and tuple(areas.shape) == (0,)


def test_fp32_set_rule(ops):
    """-1.0, -0.0, NaN and 0.5 in one plane: only 0.5 counts (the `> 0` of psalm_binarize_gather)"""
    m = np.zeros((2, 9, 21), np.float32)
    m[0, 1, 2], m[0, 2, 19], m[0, 7, 0], m[0, 4, 11] = -1.0, -0.0, np.nan, 0.5
    m[1, :, :] = np.nan
    m[1, 8, 20] = 1e-30
    t = torch.from_numpy(m).to(ops.device)
    boxes, areas = ops.mask_boxes(t)
    assert boxes.tolist() == [[11, 4, 12, 5], [20, 8, 21, 9]] and areas.tolist() == [1, 1]
    wb, wa = np_boxes(m, True)
    assert np.array_equal(boxes.cpu().numpy(), wb) and np.array_equal(areas.cpu().numpy(), wa)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "u8"])
def test_index_list(ops, dtype):
    """[2, 0, 2, -1, 99] over 3 planes: rows 2, 0, 2, empty, empty -- and the outputs written into views of a caller's block"""
    m = blobs(3, 40, 90, 3)
    check(ops, m, dtype, index=[2, 0, 2, -1, 99])
    t = torch.from_numpy(m).to(ops.device).to(dtype)
    block = torch.full((5 * 5,), -7, dtype=torch.int32, device=ops.device)
    ob, oa = block[:20].view(torch.float32).view(5, 4), block[20:]
    rb, ra = ops.mask_boxes(t, index=torch.tensor([2, 0, 2, -1, 99], dtype=torch.int32, device=ops.device), out_boxes=ob, out_areas=oa)
    assert rb.data_ptr() == ob.data_ptr() and ra.data_ptr() == oa.data_ptr()
    wb, wa = np_boxes(m, dtype == torch.float32)
    assert np.array_equal(ob.cpu().numpy(), np.stack([wb[2], wb[0], wb[2], np.zeros(4), np.zeros(4)]).astype(np.float32))
    assert oa.tolist() == [int(wa[2]), int(wa[0]), int(wa[2]), 0, 0]
    # no plane at all, an index list all the same: every row empty
    rb, ra = ops.mask_boxes(torch.zeros(0, 4, 4, dtype=dtype, device=ops.device), index=torch.tensor([0, 1], dtype=torch.int32, device=ops.device))
    assert rb.tolist() == [[0.0] * 4] * 2 and ra.tolist() == [0, 0]


def np_table(lab, n_ids):
    t = np.zeros((n_ids, 5), np.int32)
    for v in range(n_ids):
        ys, xs = np.nonzero(lab == v)
        if len(ys):
            t[v] = [xs.min(), ys.min(), xs.max() + 1, ys.max() + 1, len(ys)]
    return t


def label_map(dtype):
    """(70, 150) with ids {0, 1, 5, 255}: 0 the background, 1 a rectangle across the 64-pixel boundary, 5 two separate pieces, 255 a corner pixel
    and a column; 3 does not occur"""
    lab = np.zeros((70, 150), np.int64)
    lab[10:30, 50:140] = 1
    lab[40:45, 3:9] = 5
    lab[60:69, 120:150] = 5
    lab[0, 0] = 255
    lab[5:66, 149] = 255
    return lab.astype(dtype)


@pytest.mark.parametrize("dtype", [np.int32, np.uint8], ids=["i32", "u8"])
@pytest.mark.parametrize("n_ids", [1, 6, 256])
def test_label_boxes(ops, dtype, n_ids):
    lab = label_map(dtype)
    t = torch.from_numpy(lab).to(ops.device)
    tab = ops.label_boxes(t, n_ids)
    want = np_table(lab, n_ids)                            # n_ids = 1, 6: the values 5 / 255 >= n_ids are ignored; id 3 (and 2, 4) absent: zeros
    assert tab.dtype == torch.int32 and tuple(tab.shape) == (n_ids, 5)
    assert np.array_equal(tab.cpu().numpy(), want), (tab.cpu().numpy()[:6], want[:6])
    if n_ids >= 6:
        assert want[3].tolist() == [0] * 5 and want[5].tolist() == [3, 40, 150, 69, 5 * 6 + 9 * 30 - 6]     # (255 takes six pixels of its last column)
    again = ops.label_boxes(t, n_ids)
    assert tab.cpu().numpy().tobytes() == again.cpu().numpy().tobytes()


def test_label_boxes_negative_and_out_view(ops):
    """int32 values below 0 and above n_ids are ignored; the table may be a view of a caller's block"""
    lab = label_map(np.int32)
    lab[20:25, 60:70] = -3
    lab[33, 100:110] = 1000
    block = torch.full((4 + 6 * 5,), -1, dtype=torch.int32, device=ops.device)
    out = block[4:].view(6, 5)
    tab = ops.label_boxes(torch.from_numpy(lab).to(ops.device), 6, out=out)
    assert tab.data_ptr() == out.data_ptr() and block[:4].tolist() == [-1] * 4
    assert np.array_equal(out.cpu().numpy(), np_table(lab, 6))


def test_label_boxes_several_blocks(ops):
    """(300, 200) int32: more rows than one block's share, ids that change inside a 64-pixel segment"""
    g = np.random.default_rng(5)
    lab = g.integers(0, 12, (300 // 10, 200 // 5)).repeat(10, 0).repeat(5, 1).astype(np.int32)
    tab = ops.label_boxes(torch.from_numpy(lab).to(ops.device), 10)
    assert np.array_equal(tab.cpu().numpy(), np_table(lab, 10))


def test_errors(ops):
    f = torch.zeros(2, 8, 8, device=ops.device)
    with pytest.raises(PsalmHipError, match="float32 / uint8 / bool"):
        ops.mask_boxes(f.to(torch.int32))
    with pytest.raises(PsalmHipError, match="float32 / uint8 / bool"):
        ops.mask_boxes(f[0])
    with pytest.raises(PsalmHipError, match="contiguous"):
        ops.mask_boxes(f.permute(0, 2, 1))
    with pytest.raises(PsalmHipError, match="index"):
        ops.mask_boxes(f, index=torch.zeros(2, dtype=torch.int64, device=ops.device))
    with pytest.raises(PsalmHipError, match="out_boxes"):
        ops.mask_boxes(f, out_boxes=torch.zeros(3, 4, device=ops.device))
    with pytest.raises(PsalmHipError, match="workspace"):
        ops.mask_boxes(f, workspace=torch.zeros(2 * 5 * 4 - 1, dtype=torch.uint8, device=ops.device))
    ops.mask_boxes(f, workspace=torch.zeros(2 * 5 * 4, dtype=torch.uint8, device=ops.device))
    lab = torch.zeros(8, 8, dtype=torch.int32, device=ops.device)
    with pytest.raises(PsalmHipError, match="int32 / uint8"):
        ops.label_boxes(lab.to(torch.int64), 4)
    with pytest.raises(PsalmHipError, match="contiguous"):
        ops.label_boxes(lab.t()[:, :4], 4)
    for bad in (0, 257):
        with pytest.raises(PsalmHipError, match="n_ids"):
            ops.label_boxes(lab, bad)
    with pytest.raises(PsalmHipError, match="out"):
        ops.label_boxes(lab, 4, out=torch.zeros(4, 4, dtype=torch.int32, device=ops.device))


def test_evalout_entry_points(ops):
    """psalm_amd.evalout.mask_boxes / label_boxes: the module's `_on_device` rules -- a wrong dtype raises, bool masks are bytes, host tensors are
    moved to the binding's device"""
    from psalm_amd import evalout as E
    m = blobs(3, 20, 45, 7)
    wb, wa = np_boxes(m, False)
    for t in (torch.from_numpy(m), torch.from_numpy(m != 0), torch.from_numpy(m).float()):
        boxes, areas = E.mask_boxes(t, ops=ops)                        # (a host tensor, whatever the backend)
        assert boxes.device.type == ops.device.type and np.array_equal(boxes.cpu().numpy(), wb) and np.array_equal(areas.cpu().numpy(), wa)
    lab = label_map(np.uint8)
    tab = E.label_boxes(torch.from_numpy(lab), 256, ops=ops)
    assert tab.device.type == ops.device.type and np.array_equal(tab.cpu().numpy(), np_table(lab, 256))
    for bad in (torch.from_numpy(m).to(torch.int32), torch.from_numpy(m).double(), m):
        with pytest.raises(PsalmHipError, match="mask_boxes"):
            E.mask_boxes(bad, ops=ops)
    with pytest.raises(PsalmHipError, match="mask_boxes"):
        E.mask_boxes(torch.from_numpy(m)[0], ops=ops)
    with pytest.raises(PsalmHipError, match="label_boxes"):
        E.label_boxes(torch.from_numpy(lab).float(), 4, ops=ops)
    with pytest.raises(PsalmHipError, match="label_boxes"):
        E.label_boxes(torch.from_numpy(lab)[None], 4, ops=ops)
