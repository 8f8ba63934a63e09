"""VideoTracker (psalm_amd/video.py: the reference's DAVIS loop with memory, state on the device) on the tiny region model, kernels in the host
emulation.  The yardstick is the existing public path: `PSALM.eval_video` with the memory frame as `vp_images` and Pillow's `apply_segmentation`
of the memory masks as the prompt, plus the driver's bookkeeping restated in numpy (tests/video_util.py).  Both sides run the same kernels on one
image, so every comparison is bit for bit."""
import numpy as np
import pytest
import torch

from ops_backend import make_ops
from psalm_amd import VideoTracker, default_region_index_sampler
from psalm_amd.config import PsalmConfig
from psalm_amd.model import PSALM, default_region_point_sampler
from psalm_amd.preprocess import apply_segmentation
from psalm_amd.synthetic import make_state_dict, video_clip_inputs
from video_util import assert_same_frame, assert_same_result, host_loop, np_frame, with_prompt

_MODELS = {}


def model_for(kind, precision, task="region", **cfg_kw):
    key = (kind, precision, task, tuple(sorted(cfg_kw.items())))
    if key not in _MODELS:
        cfg = PsalmConfig.tiny(task).replace(**cfg_kw) if cfg_kw else PsalmConfig.tiny(task)
        _MODELS[key] = PSALM(cfg, make_state_dict(cfg, seed=12), ops=make_ops(kind), precision=precision)
    return _MODELS[key]


def disc(h, w, cy, cx, r):
    yy, xx = np.mgrid[:h, :w]
    return (((yy - cy) ** 2 + (xx - cx) ** 2) <= r * r).astype(np.uint8)


def crafted(model, masks_u8, at, Q=None):
    """pred_masks (Q,H,W) / scores (Q,R) in which object r's best query is at[r] and holds masks_u8[r]; every other query is empty and scores low"""
    Q = Q or model.cfg.md_queries
    R = len(masks_u8)
    pm = np.zeros((Q,) + masks_u8[0].shape, np.float32)
    sc = np.full((Q, R), 0.01, np.float32) + np.arange(Q, dtype=np.float32)[:, None] * 1e-4
    for r, (m, q) in enumerate(zip(masks_u8, at)):
        pm[q] = m
        sc[q, r] = 0.9
    dev = model.device
    return torch.from_numpy(pm).to(dev), torch.from_numpy(sc).to(dev)


def frame_tokens(model, images):
    """the projector tokens of a frame, as a step on that frame computes them"""
    f = model.swin(images.to(model.device, torch.float32).contiguous())
    return model.projector(f[3][0], 1, f[3][1], f[3][2])[0]


def memory_path_case(model, seed=7, calls=None):
    """Item 1: two disjoint discs put into the memory through the tracker's own update routine; then a step must be prompted from memory and equal
    eval_video(vp_images = memory frame, vp_region_masks = apply_segmentation(discs)) under the same RNG state, in every returned tensor."""
    f0, f1 = video_clip_inputs(model.cfg, 2, 2)
    tr = f0["seg_info"][0]["transforms"]
    h, w = tr["resize"][:2]
    discs = [disc(h, w, 20, 22, 9), disc(h, w, 40, 58, 11)]
    trk = VideoTracker(model)
    up = trk._observe(frame_tokens(model, f0["images"]), *crafted(model, discs, (3, 7)), [1, 2], tr)
    assert up["memory_updated"] and up["picked_query"].tolist() == [3, 7] and trk._mem is not None
    lib = model.ops.lib
    try:                                            # (`calls`: the library's launch records of both sides, for the launch-count test)
        lib.calls = [] if calls is not None else None
        torch.manual_seed(seed)
        out = trk.step(**f1)
        if calls is not None:
            calls["step"], lib.calls = lib.calls, []
        assert out["used_memory"] is True and trk.memory_frames == 1 and trk.prompt_frames == 0
        torch.manual_seed(seed)
        want = model.eval_video(**with_prompt(f1, f0["images"], [apply_segmentation(d, tr) for d in discs], [1, 2]))[0]
        if calls is not None:
            calls["eval_video"] = lib.calls
    finally:
        lib.calls = None
    assert_same_result(out, want)
    fr = np_frame(want["instances"].pred_masks.cpu().numpy(), want["instances"].scores.cpu().numpy(), [1, 2])
    assert out["picked_query"].tolist() == fr["query"] and np.array_equal(out["fused"].cpu().numpy(), fr["fused"])
    return out


def clip_case(model, frames=3):
    """Item 2: a clip through the tracker and through the host loop over eval_video; identical on every frame whichever branches are taken.
    Returns the branches."""
    seeds = [100 + t for t in range(frames)]
    want = host_loop(model, video_clip_inputs(model.cfg, frames, 2), seeds)
    trk = VideoTracker(model)
    taken = []
    for inputs, seed, fr in zip(video_clip_inputs(model.cfg, frames, 2), seeds, want):
        torch.manual_seed(seed)
        out = trk.step(**inputs)
        assert_same_frame(out, fr)
        taken.append((out["used_memory"], out["memory_updated"]))
    assert taken[0][0] is False                     # the first frame has no memory to be prompted from
    assert trk.memory_frames + trk.prompt_frames == frames
    return taken


_CALLS = {}


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_memory_path_equals_eval_video_on_the_memory_frame(precision):
    memory_path_case(model_for("emu", precision), calls=_CALLS.setdefault(precision, {}))


def test_memory_step_runs_one_vision_pass():
    """Item 5, from the library's launch records of the f16x3 case above (the mode whose vision tower is one native call): a memory-path step issues
    ONE psalm_swin_forward / psalm_projector_forward, the same frame through eval_video two of each; the step's bookkeeping is the four video
    entries, once each."""
    if "f16x3" not in _CALLS:
        memory_path_case(model_for("emu", "f16x3"), calls=_CALLS.setdefault("f16x3", {}))
    step_calls, video_calls = _CALLS["f16x3"]["step"], _CALLS["f16x3"]["eval_video"]
    assert step_calls.count("psalm_swin_forward") == 1 and step_calls.count("psalm_projector_forward") == 1
    assert video_calls.count("psalm_swin_forward") == 2 and video_calls.count("psalm_projector_forward") == 2
    for name in ("psalm_video_pick", "psalm_video_fuse", "psalm_mask_resize_nearest_pad", "psalm_mask_select_points"):
        assert step_calls.count(name) == 1 and video_calls.count(name) == 0, name


def test_three_frame_clip_equals_the_host_loop(record_property):
    """(fp32 here: a third of the emulator's time per frame; tests/test_15_video_tracker_gpu.py runs the clip in f16x3)"""
    taken = clip_case(model_for("emu", "fp32"))
    record_property("branches (used_memory, memory_updated) per frame", str(taken))
    print("branches (used_memory, memory_updated) per frame:", taken)


def test_index_sampler_draws_what_the_point_sampler_draws():
    """same indices and the same global-RNG state afterwards, for m < n, m == n, m > n; m == 0 fails as the reference's randint(0, 0) does"""
    with pytest.raises(RuntimeError):
        default_region_index_sampler(0, 16)
    for m in (5, 16, 400):
        torch.manual_seed(3)
        a, ra = default_region_index_sampler(m, 16), torch.rand(1)
        torch.manual_seed(3)
        b, rb = default_region_point_sampler(torch.zeros(m, 2), 16), torch.rand(1)
        assert torch.equal(a, b) and torch.equal(ra, rb)


def test_branches():
    """Item 3, with crafted scores and masks through the update routine, the prompt side through `step`."""
    model = model_for("emu", "fp32")
    clip = video_clip_inputs(model.cfg, 2, 2)
    tr = clip[0]["seg_info"][0]["transforms"]
    h, w = tr["resize"][:2]
    tok = torch.zeros(9, model.cfg.hidden_size, device=model.device)          # (the memory's tokens are not pooled from in this test)
    a, b = disc(h, w, 20, 22, 9), disc(h, w, 40, 58, 11)
    trk = VideoTracker(model)
    # accept
    up = trk._observe(tok, *crafted(model, [a, b], (3, 7)), [1, 2], tr)
    first = trk._mem
    assert up["memory_updated"] and first is not None and first.fill == [1, 2]
    assert first.counts == [int(apply_segmentation(m, tr).sum()) for m in (a, b)]
    assert np.array_equal(first.masks.cpu().numpy(), np.stack([apply_segmentation(m, tr) for m in (a, b)]))
    # reject by IoU: two discs one pixel apart overlap far above 0.4 -> the memory is kept
    up = trk._observe(tok, *crafted(model, [a, disc(h, w, 20, 23, 9)], (2, 5)), [1, 2], tr)
    assert not up["memory_updated"] and trk._mem is first and trk.rejected_updates == 1
    assert int(up["pair_inter"][0, 1]) * 5 > int(up["pair_union"][0, 1]) * 2
    # empty picked mask: the memory is left unchanged (the documented deviation), and it is not counted as a rejection
    up = trk._observe(tok, *crafted(model, [a, np.zeros_like(a)], (4, 6)), [1, 2], tr)
    assert not up["memory_updated"] and trk._mem is first and trk.rejected_updates == 1 and trk.empty_updates == 1
    # object-count mismatch: three objects against a memory of two -> the caller's prompt
    three = video_clip_inputs(model.cfg, 1, 3)[0]
    trk._video = "clip0"
    out = trk.step(**three)
    assert out["used_memory"] is False and trk.prompt_frames == 1 and out["picked_masks"].shape[0] == 3
    # directory change -> reset: a memory of two objects is NOT used for a two-object frame of another clip
    trk2 = VideoTracker(model)
    trk2._observe(tok, *crafted(model, [a, b], (3, 7)), [1, 2], tr)
    trk2._video = "clip0"
    other = video_clip_inputs(model.cfg, 1, 2, clip="clip1")[0]
    out = trk2.step(**other)
    assert out["used_memory"] is False and trk2._video == "clip1" and trk2.memory_frames == 0
    # reset() forgets memory and clip
    trk.reset()
    assert trk._mem is None and trk._video is None


def test_errors():
    model = model_for("emu", "f16x3")
    clip = video_clip_inputs(model.cfg, 1, 2)
    tr = clip[0]["seg_info"][0]["transforms"]
    h, w = tr["resize"][:2]
    a, b = disc(h, w, 20, 22, 9), disc(h, w, 40, 58, 11)
    tok = torch.zeros(4, model.cfg.hidden_size, device=model.device)
    trk = VideoTracker(model)
    with pytest.raises(ValueError, match="Q = 9"):                      # torch.topk(..., 10) of fewer than ten scores
        trk._observe(tok, *crafted(model, [a, b], (3, 7), Q=9), [1, 2], tr)
    with pytest.raises(ValueError, match="0..255"):
        trk._observe(tok, *crafted(model, [a, b], (3, 7)), [1, 256], tr)
    with pytest.raises(ValueError, match="at most 32"):
        trk._observe(tok, *crafted(model, [a] * 33, list(range(12)) * 2 + list(range(9))), list(range(33)), tr)
    bad = clip[0]["seg_info"][0]["instances"]
    bad.vp_fill_number = torch.tensor([1, 256])
    with pytest.raises(ValueError, match="0..255"):
        trk.step(**clip[0])
    with pytest.raises(ValueError, match="Q = 8"):
        VideoTracker(model_for("emu", "f16x3", md_queries=8))
    with pytest.raises(ValueError, match="region"):
        VideoTracker(model_for("emu", "f16x3", task="referring"))
    assert trk._mem is None and trk.memory_frames == trk.prompt_frames == 0
