"""Video object tracking: `VideoTracker.step` per frame against the host loop over `PSALM.eval_video` (the reference's DAVIS driver with memory).

    python tools/bench_video.py [--frames 20] [--reps 5] [--warmup 1] [--layers 24] [--out profiles/video_track_bench.json]

Full synthetic region model, precision "f16x3", one synthetic clip: 480 x 854 frames resized and padded into the 1024^2 canvas as the instance
pre-processor does, 3 objects.  A random model's picks rarely pass the driver's IoU check, so the memory is seeded once with three disjoint discs
(through the tracker's own update routine; the same discs for the host loop): from then on every frame is prompted from memory on both sides, and
whether a frame REPLACES the memory is left to the model, identically on both sides.
  tracker      VideoTracker.step: one vision pass per frame, bookkeeping on the device, one small read-back
  host_eager   eval_video(vp_images = memory frame) + all Q masks to the host + numpy pick / IoU / fuse + Pillow resize of the memory masks
  host_graphs  the same with use_graphs=True (eval_video's best form)
All three in this process on this device.  A repetition = the whole clip, wall time with a final synchronize; frames/s from the median of `--reps`
repetitions after `--warmup`.  Also the bytes each side copies device-to-host per frame.  One JSON with the commit hash is written to --out.
"""
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


def disc(h, w, cy, cx, r):
    yy, xx = np.mgrid[:h, :w]
    return (((yy - cy) ** 2 + (xx - cx) ** 2) <= r * r).astype(np.uint8)


def host_clip(model, clip, mem, stats):
    """the driver's loop (eval_davis.py:388-480) on the host; mem = [image, masks at the original size, fill, transforms]"""
    from psalm_amd.preprocess import apply_segmentation
    from psalm_amd.synthetic import RegionInstances
    mem = list(mem)
    for inputs in clip:
        info = dict(inputs["seg_info"][0])
        old = info["instances"]
        vp = torch.from_numpy(np.stack([apply_segmentation(m, mem[3]) for m in mem[1]]))
        inst = RegionInstances(old.region_masks.tensor, old.gt_masks, vp)
        inst.vp_fill_number = torch.tensor(mem[2])
        info["instances"] = inst
        res = model.eval_video(input_ids=inputs["input_ids"], attention_mask=inputs["attention_mask"], images=inputs["images"], vp_images=mem[0],
                               seg_info=[info], labels=inputs["labels"])[0]
        pm = res["instances"].pred_masks.cpu().numpy()
        sc = res["instances"].scores.cpu().numpy().T
        stats["d2h"] = pm.nbytes + sc.nbytes
        taken, masks = [], []
        q_now = 0
        for r in range(sc.shape[0]):
            for q in np.argsort(-sc[r], kind="stable")[:10]:
                if int(q) not in taken:
                    taken.append(int(q))
                    q_now = int(q)
                    break
            masks.append(pm[q_now].astype(np.uint8))
        fused = np.zeros_like(masks[0])
        for m, f in zip(masks, mem[2]):
            fused[m == 1] = f
        ok = True
        for i in range(len(masks)):
            for j in range(len(masks)):
                if i != j:
                    u = np.logical_or(masks[i], masks[j]).sum()
                    if u and np.logical_and(masks[i], masks[j]).sum() / u > 0.4:
                        ok = False
        if ok and all(m.any() and apply_segmentation(m, info["transforms"]).any() for m in masks):
            mem = [inputs["images"], masks, mem[2], info["transforms"]]
            stats["updates"] = stats.get("updates", 0) + 1


def run(fn, reps, warmup, frames):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    wall = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        wall.append(time.perf_counter() - t)
    med = statistics.median(wall)
    return {"frames_per_s": round(frames / med, 3), "ms_per_frame_median": round(med / frames * 1e3, 3),
            "ms_per_frame_min": round(min(wall) / frames * 1e3, 3), "ms_per_frame_max": round(max(wall) / frames * 1e3, 3), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--objects", type=int, default=3)
    ap.add_argument("--commit", default=None, help="commit hash to record (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "video_track_bench.json"))
    args = ap.parse_args()
    from psalm_amd import VideoTracker
    from psalm_amd.config import PsalmConfig
    from psalm_amd.model import PSALM
    from psalm_amd.synthetic import make_state_dict, video_clip_inputs
    cfg = PsalmConfig(num_layers=args.layers, seg_task="region")
    model = PSALM(cfg, make_state_dict(cfg, seed=1), precision="f16x3", use_graphs=False)
    h, w, R = 480, 854, args.objects
    clip = video_clip_inputs(cfg, args.frames + 1, R, size=args.size, orig=(h, w), seed=1)
    for d in clip:
        d["images"] = d["images"].cuda()
        d["vp_images"] = d["vp_images"].cuda()
    seed_frame, clip = clip[0], clip[1:]
    tr = seed_frame["seg_info"][0]["transforms"]
    discs = [disc(h, w, 120 + 110 * (r % 3), 150 + 180 * (r % 4), 40) for r in range(R)]
    fill = list(range(1, R + 1))
    Q = cfg.md_queries
    pm = torch.zeros(Q, h, w)
    sc = torch.full((Q, R), 0.01)
    for r in range(R):
        pm[r] = torch.from_numpy(discs[r])
        sc[r, r] = 0.9
    pm, sc = pm.cuda(), sc.cuda()
    f = model.swin(seed_frame["images"])
    tokens = model.projector(f[3][0], 1, f[3][1], f[3][2])[0]
    trk = VideoTracker(model)

    def tracker_clip():
        trk.reset()
        assert trk._observe(tokens, pm, sc, fill, tr)["memory_updated"]
        for d in clip:
            trk.step(**d)

    stats = {}
    mem = [seed_frame["images"], discs, fill, tr]
    commit = args.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    res = {"commit": commit, "device": torch.cuda.get_device_name(0), "precision": "f16x3", "layers": args.layers, "frames": args.frames,
           "frame": [h, w], "canvas": args.size, "objects": R}
    torch.manual_seed(0)
    res["tracker"] = run(tracker_clip, args.reps, args.warmup, args.frames)
    res["tracker"]["d2h_bytes_per_frame"] = 4 * (1 + 4 * R + 2 * R * R)
    res["tracker"]["counters"] = {k: getattr(trk, k) for k in ("memory_frames", "prompt_frames", "rejected_updates", "empty_updates")}
    torch.manual_seed(0)
    res["host_eager"] = run(lambda: host_clip(model, clip, mem, stats), args.reps, args.warmup, args.frames)
    res["host_eager"]["d2h_bytes_per_frame"] = stats["d2h"]
    model.use_graphs = True
    try:
        torch.manual_seed(0)
        res["host_graphs"] = run(lambda: host_clip(model, clip, mem, stats), args.reps, max(args.warmup, 2), args.frames)
        res["host_graphs"]["d2h_bytes_per_frame"] = stats["d2h"]
    finally:
        model.use_graphs = False
        model._graphs.clear()
    res["tracker_not_slower"] = {k: res["tracker"]["frames_per_s"] >= res[k]["frames_per_s"] for k in ("host_eager", "host_graphs")}
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
