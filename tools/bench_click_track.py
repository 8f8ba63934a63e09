"""Prompt-driven video tracking: `VideoTracker.start` / `track` against `VideoTracker.step` fed with a host-prepared dataset record.

    python tools/bench_click_track.py [--frames 20] [--warmup 3] [--layers 24] [--out profiles/click_track_bench.json]

Full synthetic region model, precision "f16x3", eager launches, one process, one device.  Every frame is timed on its own (synchronize, call,
synchronize), the two sides alternate frame by frame, and the state both sides start a frame from is set outside the timed span; the figure is the
median over `--frames` frames after `--warmup`.
  origin   an origin-path `track` frame (memory emptied before every frame) against a `step` frame prompted from `vp_images` / `vp_region_masks`
           (memory emptied likewise): 3 objects, 480 x 854 frames in the 1024^2 canvas
  memory   a memory-path `track` frame against a memory-path `step` frame, the memory seeded with three disjoint discs before every frame: the control
  start    `start` with 1 and 3 clicks against host preparation (draw the click, enhance_with_circles, apply_segmentation, an `instances` record with a
           stand-in `gt_masks`) + `step` on an empty tracker, at 480 x 854 and 1024 x 1024 originals; the host preparation is also given alone
One JSON with the commit hash is written to --out."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GEOMETRY = ("padding_mask", "height", "width", "transforms")


def disc(h, w, cy, cx, r):
    yy, xx = np.mgrid[:h, :w]
    return (((yy - cy) ** 2 + (xx - cx) ** 2) <= r * r).astype(np.uint8)


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def summary(ms, warmup):
    ms = ms[warmup:]
    return {"ms_median": round(statistics.median(ms), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3), "frames": len(ms)}


def pair(a, b):
    a = dict(a)
    a["saved_ms"] = round(b["ms_median"] - a["ms_median"], 3)
    return a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--commit", default=None, help="commit hash to record (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "click_track_bench.json"))
    args = ap.parse_args()
    from psalm_amd import VideoTracker
    from psalm_amd.config import PsalmConfig
    from psalm_amd.model import PSALM
    from psalm_amd.preprocess import apply_segmentation, enhance_with_circles
    from psalm_amd.synthetic import RegionInstances, make_state_dict, video_clip_inputs
    cfg = PsalmConfig(num_layers=args.layers, seg_task="region")
    model = PSALM(cfg, make_state_dict(cfg, seed=1), precision="f16x3", use_graphs=False)
    n = args.frames + args.warmup
    commit = args.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    res = {"commit": commit, "device": torch.cuda.get_device_name(0), "precision": "f16x3", "layers": args.layers, "canvas": args.size,
           "frames": args.frames, "warmup": args.warmup, "timing": "per frame, synchronized, sides alternating; medians"}

    def clip_for(R, orig):
        clip = video_clip_inputs(cfg, n + 1, R, size=args.size, orig=orig, seed=1)
        for d in clip:
            d["images"] = d["images"].cuda()
            d["vp_images"] = d["vp_images"].cuda()
        return clip

    def geometry(d):
        return [{k: d["seg_info"][0][k] for k in GEOMETRY}]

    def clicks(R, h, w):
        return [{"points": [(h // 4 + (h // 5) * (r % 3), w // 5 + (w // 4) * (r % 3))]} for r in range(R)]

    def host_record(d, regions, tr, h, w):
        """what a caller of `step` prepares on the host for these clicks"""
        vp = []
        for rp in regions:
            m = np.zeros((h, w), np.uint8)
            for y, x in rp["points"]:
                m[y, x] = 1
            vp.append(apply_segmentation(enhance_with_circles(m, 10), tr))
        vp = torch.from_numpy(np.stack(vp))
        inst = RegionInstances(vp, vp.float(), vp)
        inst.vp_fill_number = torch.arange(1, len(regions) + 1)
        info = dict(geometry(d)[0], instances=inst)
        return dict(d, seg_info=[info], vp_images=d["images"])

    # ---- origin-path and memory-path frames: 3 objects, 480 x 854
    h, w, R = 480, 854, 3
    clip = clip_for(R, (h, w))
    first, rest = clip[0], clip[1:]
    tr = first["seg_info"][0]["transforms"]
    regions = clicks(R, h, w)
    trk, ref = VideoTracker(model), VideoTracker(model)
    trk.start(first["input_ids"], first["images"], geometry(first), regions=regions, attention_mask=first["attention_mask"])
    origin, prompt = trk._origin, trk._prompt
    proto = host_record(first, regions, tr, h, w)["seg_info"][0]["instances"]
    a, b = [], []
    for d in rest:
        trk._mem = ref._mem = None
        a.append(timed(lambda: trk.track(d["images"], geometry(d)))[0])
        ref._mem = None
        b.append(timed(lambda: ref.step(**dict(d, vp_images=first["images"], seg_info=[dict(d["seg_info"][0], instances=proto)])))[0])
    assert trk.memory_frames == 0 and ref.memory_frames == 0
    res["origin"] = {"objects": R, "frame": [h, w], "track": pair(summary(a, args.warmup), summary(b, args.warmup)), "step": summary(b, args.warmup)}

    discs = [disc(h, w, 120 + 110 * r, 150 + 180 * r, 40) for r in range(R)]
    Q = cfg.md_queries
    pm, sc = torch.zeros(Q, h, w), torch.full((Q, R), 0.01)
    for r in range(R):
        pm[r] = torch.from_numpy(discs[r])
        sc[r, r] = 0.9
    pm, sc = pm.cuda(), sc.cuda()
    f = model.swin(first["images"])
    tokens = model.projector(f[3][0], 1, f[3][1], f[3][2])[0]
    a, b = [], []
    for d in rest:
        for t in (trk, ref):
            t._mem = None
            assert t._observe(tokens, pm, sc, [1, 2, 3], tr)["memory_updated"]
        a.append(timed(lambda: trk.track(d["images"], geometry(d)))[0])
        b.append(timed(lambda: ref.step(**d))[0])
    assert trk.memory_frames == len(rest) and ref.memory_frames == len(rest) and trk._origin is origin and trk._prompt is prompt
    res["memory"] = {"objects": R, "frame": [h, w], "track": pair(summary(a, args.warmup), summary(b, args.warmup)), "step": summary(b, args.warmup)}

    # ---- start against host preparation + step
    res["start"] = []
    for orig in ((480, 854), (1024, 1024)):
        for R in (1, 3):
            h, w = orig
            clip = clip_for(R, orig)[:n]
            regions = clicks(R, h, w)
            a, b, p = [], [], []
            for d in clip:
                tr = d["seg_info"][0]["transforms"]
                a.append(timed(lambda: trk.start(d["input_ids"], d["images"], geometry(d), regions=regions, attention_mask=d["attention_mask"]))[0])
                ref._mem = None
                t0 = time.perf_counter()
                rec = host_record(d, regions, tr, h, w)
                p.append((time.perf_counter() - t0) * 1e3)
                b.append(p[-1] + timed(lambda: ref.step(**rec))[0])
            res["start"].append({"clicks": R, "frame": [h, w], "start": pair(summary(a, args.warmup), summary(b, args.warmup)),
                                 "host_prep_plus_step": summary(b, args.warmup), "host_prep_alone": summary(p, args.warmup)})
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
