"""Helpers of the prompt-driven tracking tests (tests/test_26_click_track_emu.py, tests/test_27_click_track_gpu.py): `VideoTracker.start` / `track` /
`adopt` against the existing public `VideoTracker.step` fed with the host-prepared dataset record they replace -- the prompt drawn in numpy
(interactive_util.mask_of), apply_segmentation, `vp_region_masks` / `vp_fill_number` / `vp_images` through video_util.with_prompt.  Both sides run the
same kernels on the same inputs, so every comparison is bit for bit.  Tiny region model, canvas 96, originals (60, 80) and (80, 60): the resize to
72 x 96 (96 x 72) + pad is not the identity, so original-pixel and canvas coordinates cannot be mixed up unseen."""
import copy

import numpy as np
import pytest
import torch

from interactive_util import CountingSampler, blob, line, mask_of, model_for
from psalm_amd import VideoTracker
from psalm_amd.config import REGION_TOKEN_INDEX
from psalm_amd.preprocess import apply_segmentation, nearest_pad_tables
from psalm_amd.synthetic import video_clip_inputs
from test_14_video_tracker_emu import crafted, disc, frame_tokens
from video_util import with_prompt

GEOMETRY = ("padding_mask", "height", "width", "transforms")
COUNTERS = ("memory_frames", "prompt_frames", "rejected_updates", "empty_updates")
HOST_KEYS = ("picked_query", "picked_scores", "pair_inter", "pair_union")
MASK_LAUNCHES = ("psalm_mask_rasterize", "psalm_mask_dilate_disc", "psalm_mask_resize_nearest_pad", "psalm_mask_select_points")


def geometry(frame):
    """what `start` / `track` need of a frame's seg_info: no instances, no file name"""
    return [{k: frame["seg_info"][0][k] for k in GEOMETRY}]


def prompts_for(R, h, w, device):
    """R = 1: one click; R = 2: click + box; R = 3: box + scribble + bool mask on the device"""
    if R == 1:
        return [{"points": [(h // 2, w // 3)]}]
    if R == 2:
        return [{"points": [(h // 3, w // 4)], "radius": 7}, {"box": (h // 2, w // 2, h - 4, w - 3)}]
    return [{"box": (h // 6, w // 4, h // 2, w)}, {"scribble": line(5, 5, h - 10, w - 10, 40)}, {"mask": torch.from_numpy(blob(h, w) != 0).to(device)}]


def host_prompt(frame, first, regions, fill):
    """the frame's inputs for the yardstick `step`: the prompt masks prepared on the host, the clip's first frame as `vp_images`"""
    tr = first["seg_info"][0]["transforms"]
    h, w = tr["resize"][:2]
    return with_prompt(frame, first["images"], [apply_segmentation(mask_of(rp, h, w), tr) for rp in regions], fill)


def counters(trk):
    return {k: getattr(trk, k) for k in COUNTERS}


def assert_same_track(got, want, used_memory=True):
    """a result of `start` / `track` against the yardstick step's: every key of the contract, bit for bit; no `gt`"""
    assert "gt" not in got and set(got) == set(want) - {"gt"}
    assert torch.equal(got["mask_pred"].cpu(), want["mask_pred"].cpu())
    gi, wi = got["instances"], want["instances"]
    assert gi.image_size == wi.image_size and set(gi.get_fields()) == set(wi.get_fields())
    for k, v in wi.get_fields().items():
        assert torch.equal(gi.get_fields()[k].cpu(), v.cpu()), k
    for k in ("picked_masks", "fused") + HOST_KEYS:
        assert got[k].dtype == want[k].dtype and torch.equal(got[k].cpu(), want[k].cpu()), k
    assert got["memory_updated"] == want["memory_updated"]
    if used_memory:
        assert got["used_memory"] is want["used_memory"]


def recorded(lib, calls, name, fn):
    """fn() with the library's launch records kept under calls[name] (calls None: not recorded)"""
    if calls is None:
        return fn()
    lib.calls = []
    try:
        out = fn()
        calls[name] = lib.calls
    finally:
        lib.calls = None
    return out


# ---------------------------------------------------------------------------------------------------- cases (kind: "emu" | "hip")
def start_case(kind, precision, R, orig, fill=None, calls=None):
    """Case 1: `start` == the yardstick `step` on frame 0 prompted from itself, under a sampler whose answers depend on the call order; the kept
    origin is apply_segmentation of the prompts."""
    model = model_for(kind, precision)
    f0 = video_clip_inputs(model.cfg, 1, R, orig=orig)[0]
    tr = f0["seg_info"][0]["transforms"]
    h, w = tr["resize"][:2]
    assert (h, w) == tuple(orig)
    regions = prompts_for(R, h, w, model.device)
    F = list(range(1, R + 1)) if fill is None else fill
    s1, s2 = CountingSampler(), CountingSampler()
    ref = VideoTracker(model)
    lib = model.ops.lib
    want = recorded(lib, calls, "step0", lambda: ref.step(**host_prompt(f0, f0, regions, F), region_index_sampler=s1))
    trk = VideoTracker(model)
    got = recorded(lib, calls, "start", lambda: trk.start(f0["input_ids"], f0["images"], geometry(f0), regions=regions,
                                                          attention_mask=f0["attention_mask"], fill=fill, region_index_sampler=s2))
    assert s1.calls == s2.calls and len(s1.calls) == R
    assert_same_track(got, want)
    assert got["used_memory"] is False and counters(trk) == counters(ref) and trk.prompt_frames == 1
    org = trk._origin
    host = np.stack([apply_segmentation(mask_of(rp, h, w), tr) for rp in regions])
    assert np.array_equal(org.masks.cpu().numpy(), host) and org.counts == host.reshape(R, -1).sum(1).tolist() == s1.calls
    assert np.array_equal(org.row_cnt.cpu().numpy(), host.sum(2)) and org.fill == F
    assert torch.equal(org.tokens.cpu(), frame_tokens(model, f0["images"]).cpu())
    assert (trk._mem is None) == (not got["memory_updated"])
    return got


def clip_case(kind, precision, orig=(80, 60), R=2, frames=3, calls=None):
    """Case 2: `start` + `track` == the yardstick tracker's `step`, frame by frame, whichever branches are taken.  Returns the branches."""
    model = model_for(kind, precision)
    clip = video_clip_inputs(model.cfg, frames, R, orig=orig)
    h, w = orig
    regions = prompts_for(R, h, w, model.device)
    F = [7, 200, 31][:R]
    s1, s2 = CountingSampler(), CountingSampler()
    ref, trk = VideoTracker(model), VideoTracker(model)
    lib = model.ops.lib
    taken = []
    for t, frame in enumerate(clip):
        want = recorded(lib, calls, f"step{t}", lambda: ref.step(**host_prompt(frame, clip[0], regions, F), region_index_sampler=s1))
        if t == 0:
            got = recorded(lib, calls, "start", lambda: trk.start(frame["input_ids"], frame["images"], geometry(frame), regions=regions,
                                                                  attention_mask=frame["attention_mask"], fill=F, region_index_sampler=s2))
        else:
            got = recorded(lib, calls, f"track{t}", lambda: trk.track(frame["images"], geometry(frame), region_index_sampler=s2))
        assert_same_track(got, want)
        assert s1.calls == s2.calls and counters(trk) == counters(ref)
        taken.append((got["used_memory"], got["memory_updated"]))
    assert taken[0][0] is False and trk.memory_frames + trk.prompt_frames == frames
    assert any(not used for used, _ in taken[1:]), "no frame ran the origin path"
    return taken


def memory_case(kind, precision, orig=(60, 80)):
    """Case 3: after `start`, crafted disjoint discs go into the memory through the tracker's own update routine (on both trackers); `track` is then
    a memory step and equals the yardstick's."""
    model = model_for(kind, precision)
    f0, f1 = video_clip_inputs(model.cfg, 2, 2, orig=orig)
    tr = f0["seg_info"][0]["transforms"]
    h, w = tr["resize"][:2]
    regions = prompts_for(2, h, w, model.device)
    s1, s2 = CountingSampler(), CountingSampler()
    ref, trk = VideoTracker(model), VideoTracker(model)
    ref.step(**host_prompt(f0, f0, regions, [1, 2]), region_index_sampler=s1)
    trk.start(f0["input_ids"], f0["images"], geometry(f0), regions=regions, region_index_sampler=s2)
    discs = [disc(h, w, 20, 22, 9), disc(h, w, 40, 38, 11)]
    tok = frame_tokens(model, f0["images"])
    for t in (ref, trk):
        up = t._observe(tok, *crafted(model, discs, (3, 7)), [1, 2], tr)
        assert up["memory_updated"] and t._mem is not None
    want = ref.step(**host_prompt(f1, f0, regions, [1, 2]), region_index_sampler=s1)
    got = trk.track(f1["images"], geometry(f1), region_index_sampler=s2)
    assert want["used_memory"] is True and got["used_memory"] is True
    assert_same_track(got, want)
    assert s1.calls == s2.calls and counters(trk) == counters(ref) and trk.memory_frames == 1 and trk.prompt_frames == 1
    return got


def adopt_case(kind, precision, orig=(80, 60)):
    """Case 4: crafted discs adopted on an encoded session; the kept masks are apply_segmentation of the discs, the totals their sums, and `track`
    equals `step` prompted through with_prompt(frame, session image, those masks, fill).  `adopt` makes the masks the MEMORY of the track, so the
    frame is a memory step here (`used_memory`, `memory_frames`) where the fresh yardstick tracker counts a prompt step; everything else is equal."""
    model = model_for(kind, precision)
    f0, f1 = video_clip_inputs(model.cfg, 2, 2, orig=orig)
    tr = f0["seg_info"][0]["transforms"]
    h, w = tr["resize"][:2]
    discs = [disc(h, w, 20, 22, 9), disc(h, w, 50, 38, 11)]
    host = [apply_segmentation(d, tr) for d in discs]
    sess = model.encode_image(f0["images"], geometry(f0))
    trk = VideoTracker(model)
    masks = torch.from_numpy(np.stack(discs)).to(model.device)
    assert trk.adopt(sess, masks, f0["input_ids"], f0["attention_mask"], fill=[4, 9]) is None
    assert trk._origin is trk._mem and counters(trk) == dict.fromkeys(COUNTERS, 0)
    assert np.array_equal(trk._mem.masks.cpu().numpy(), np.stack(host)) and trk._mem.counts == [int(m.sum()) for m in host]
    assert trk._mem.fill == [4, 9] and torch.equal(trk._mem.tokens.cpu(), sess.image_tokens.cpu())
    assert trk._mem.tokens.data_ptr() != sess.image_tokens.data_ptr()
    s1, s2 = CountingSampler(), CountingSampler()
    ref = VideoTracker(model)
    want = ref.step(**with_prompt(f1, f0["images"], host, [4, 9]), region_index_sampler=s1)
    got = trk.track(f1["images"], geometry(f1), region_index_sampler=s2)
    assert_same_track(got, want, used_memory=False)
    assert got["used_memory"] is True and s1.calls == s2.calls
    assert (trk.memory_frames, trk.prompt_frames) == (1, 0) and (ref.memory_frames, ref.prompt_frames) == (0, 1)
    assert (trk.rejected_updates, trk.empty_updates) == (ref.rejected_updates, ref.empty_updates)
    # bool masks from the host, default fill: the same memory
    trk2 = VideoTracker(model)
    trk2.adopt(sess, np.stack(discs) != 0, f0["input_ids"][0])
    assert torch.equal(trk2._mem.masks, trk._mem.masks) and trk2._mem.counts == trk._mem.counts and trk2._mem.fill == [1, 2]
    return got


def launches_check(calls, track="track1", step="step1"):
    """Case 5, from the launch records of an f16x3 clip (the mode whose vision tower is one native call)"""
    for name, passes in (("start", 1), (track, 1), ("step0", 2), (step, 2)):
        assert calls[name].count("psalm_swin_forward") == passes and calls[name].count("psalm_projector_forward") == passes, name
    want = dict(zip(MASK_LAUNCHES, (1, 1, 2, 1)))             # (resize + pad: the prompt's, and the one the frame's bookkeeping does)
    for name, n in want.items():
        assert calls["start"].count(name) == n, (name, calls["start"].count(name))
    assert calls[track].count("psalm_mask_rasterize") == 0 and calls[track].count("psalm_mask_dilate_disc") == 0
    assert calls[track].count("psalm_mask_select_points") == 1 and calls[track].count("psalm_mask_resize_nearest_pad") == 1
    for name in ("psalm_video_pick", "psalm_video_fuse"):
        assert calls["start"].count(name) == 1 and calls[track].count(name) == 1, name


def unchanged_case(kind, precision):
    """Case 6: a `step` clip on a tracker that went through start + track + reset() equals the clip on a fresh tracker"""
    model = model_for(kind, precision)
    clip = video_clip_inputs(model.cfg, 2, 2)
    h, w = clip[0]["seg_info"][0]["transforms"]["resize"][:2]
    used = VideoTracker(model)
    used.start(clip[0]["input_ids"], clip[0]["images"], geometry(clip[0]), regions=prompts_for(2, h, w, model.device))
    used.track(clip[1]["images"], geometry(clip[1]))
    used.reset()
    assert used._mem is None and used._origin is None
    with pytest.raises(ValueError, match="start or adopt"):
        used.track(clip[1]["images"], geometry(clip[1]))
    before = counters(used)
    fresh = VideoTracker(model)
    for t, frame in enumerate(clip):
        torch.manual_seed(50 + t)
        want = fresh.step(**frame)
        torch.manual_seed(50 + t)
        got = used.step(**frame)
        assert torch.equal(got["gt"].cpu(), want["gt"].cpu()) and set(got) == set(want)
        assert_same_track({k: v for k, v in got.items() if k != "gt"}, want)
    assert {k: getattr(used, k) - before[k] for k in COUNTERS} == counters(fresh)


def state_of(trk):
    return (trk._origin, trk._mem, trk._prompt, counters(trk))


def errors_case(kind, precision="fp32"):
    """Case 7: every error names what is wrong, and a failed `start` / `adopt` leaves origin, memory and counters as they were"""
    model = model_for(kind, precision)
    cfg = model.cfg
    f0, f1 = video_clip_inputs(cfg, 2, 2)
    tr = f0["seg_info"][0]["transforms"]
    h, w = tr["resize"][:2]
    ids, img, geo = f0["input_ids"], f0["images"], geometry(f0)
    good = prompts_for(2, h, w, model.device)
    trk = VideoTracker(model)
    with pytest.raises(ValueError, match="start or adopt"):
        trk.track(f1["images"], geometry(f1))
    trk.start(ids, img, geo, regions=good)
    sess = model.encode_image(img, geo)
    discs = np.stack([disc(h, w, 20, 22, 9), disc(h, w, 40, 58, 11)])
    state = state_of(trk)

    def start_fails(match, exc=ValueError, **kw):
        args = dict(input_ids=ids, images=img, seg_info=geo, regions=good)
        args.update(kw)
        with pytest.raises(exc, match=match):
            trk.start(**args)
        assert state_of(trk) == state

    def adopt_fails(match, session=sess, masks=discs, input_ids=ids, **kw):
        with pytest.raises(ValueError, match=match):
            trk.adopt(session, masks, input_ids, **kw)
        assert state_of(trk) == state

    three = video_clip_inputs(cfg, 1, 3)[0]["input_ids"]
    start_fails("2 regions for 3 <region> tokens", input_ids=three)
    start_fails("3 regions for 2 <region> tokens", regions=good + good[:1])
    start_fails("prompt 0, region 1: .*exactly one of", regions=[good[0], {}])
    start_fails("prompt 0, region 0: unknown keys", regions=[{"box": (0, 0, 2, 2), "radius": 3}, good[1]])
    start_fails(f"prompt 0, region 0: pixel .* outside the image of .*{h}, {w}", regions=[{"points": [(h, 0)]}, good[1]])
    start_fails("prompt 0, region 1: box", regions=[good[0], {"box": (0, 0, h + 1, w)}])
    start_fails("prompt 0, region 0: radius 17", regions=[{"points": [(1, 1)], "radius": 17}, good[1]])
    start_fails("prompt 0, region 1: a mask of shape", regions=[good[0], {"mask": np.zeros((w, h), np.uint8)}])
    start_fails("prompt 0, region 1: no pixel", regions=[good[0], {"mask": np.zeros((h, w), np.uint8)}])
    start_fails("a list with one region prompt", regions={"points": [(1, 1)]})
    start_fails("0..255", fill=[1, 256])
    start_fails("1 fill numbers for 2 regions", fill=[1])
    start_fails("batch 1", images=torch.cat([img, img]))
    start_fails("batch 1", seg_info=geo + geo)
    start_fails("batch 1", input_ids=torch.cat([ids, ids]))
    start_fails("transforms", seg_info=[{k: v for k, v in geo[0].items() if k != "transforms"}])
    start_fails("transforms lead to", seg_info=[dict(geo[0], transforms={"resize": (h, w, 60, 80), "pad": (4, 16)})])
    lst = ids[0].tolist()
    many = torch.tensor([lst[:lst.index(REGION_TOKEN_INDEX)] + [REGION_TOKEN_INDEX] * 31 + lst[lst.index(REGION_TOKEN_INDEX):]])      # 33 <region> tokens
    start_fails("at most 32", input_ids=many, regions=[good[0]] * 33)
    # a pixel that the down-scaling resize drops: 300 x 200 -> 96 x 64 reads one source row in three
    tall = video_clip_inputs(cfg, 1, 2, orig=(300, 200))[0]
    rows, cols = nearest_pad_tables(*tall["seg_info"][0]["transforms"]["resize"], *tall["seg_info"][0]["transforms"]["pad"])
    y = next(v for v in range(300) if v not in set(rows.tolist()))
    start_fails("prompt 0, region 0: no pixel of the prompt is left after the resize", images=tall["images"], seg_info=geometry(tall),
                regions=[{"points": [(y, int(cols[3]))], "radius": 0}, {"box": (0, 0, 50, 50)}])

    adopt_fails("2 regions for 3 <region> tokens", input_ids=three)
    adopt_fails("masks of shape", masks=discs.transpose(0, 2, 1))
    adopt_fails("masks of shape", masks=discs[0])
    adopt_fails("dtype", masks=discs.astype(np.float32))
    adopt_fails("region 1: no pixel", masks=np.stack([discs[0], np.zeros_like(discs[0])]))
    adopt_fails("0..255", fill=[-1, 2])
    adopt_fails("another model", session=model_for(kind, "f16x3" if precision == "fp32" else "fp32").encode_image(img, geo))
    adopt_fails("another model", session=None)
    bare = copy.copy(sess)
    bare.seg_info = {k: v for k, v in geo[0].items() if k != "transforms"}
    adopt_fails("transforms", session=bare)
    stale = copy.copy(sess)
    stale.version = sess.version + 1
    adopt_fails("weights were prepared again", session=stale)
    many_masks = np.repeat(discs[:1], 33, 0)
    adopt_fails("at most 32", masks=many_masks, input_ids=many)

    with pytest.raises(ValueError, match="batch 1"):
        trk.track(torch.cat([f1["images"]] * 2), geometry(f1))
    with pytest.raises(ValueError, match="transforms"):
        trk.track(f1["images"], [{"height": h, "width": w}])
    with pytest.raises(ValueError, match="the track began on"):
        trk.track(torch.zeros(1, 3, 64, 64), geometry(f1))
    assert state_of(trk) == state
    # bf16 / llm_products = 1: no tracker to call start on
    for kw in ({"precision": "bf16"}, {"llm_products": 1}):
        fake = type("M", (), dict({"seg_task": "region", "precision": "f16x3", "llm_products": 3, "cfg": cfg, "ops": model.ops}, **kw))()
        with pytest.raises(NotImplementedError):
            VideoTracker(fake)
