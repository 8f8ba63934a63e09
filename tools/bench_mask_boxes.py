"""Boxes and areas from masks on the device: psalm_mask_boxes / psalm_label_boxes against psalm_binarize_gather, the pass that reads the same bytes.

    python tools/bench_mask_boxes.py [--reps 30] [--inner 5] [--warmup 5] [--out profiles/mask_boxes_bench.json]

One process, one device, op-level calls on the default stream.  A sample is the device-event time around `--inner` back-to-back calls divided by
`--inner` (memset node and finishing kernel included); the cases alternate sample by sample, so they see the same machine; the figure is the median
of `--reps` samples after `--warmup`.  bytes/s = the bytes of the input the call must read (n H W x element size) over that time.
  mask_boxes_f32     (100, 1024, 1024) float32: `instances.pred_masks` of one 1024^2 image -- 419 MB, larger than the 256 MB last-level cache
  binarize_gather    the same tensor through psalm_binarize_gather (reads 419 MB, writes 419 MB): the yardstick, per byte READ
  mask_boxes_u8      (3, 480, 854) uint8: the tracker's picked masks -- 1.2 MB, cache-resident: a launch / latency figure
  label_boxes_i32    (1024, 1024) int32: a panoptic id map -- 4 MB, cache-resident likewise
The masks hold one disc per plane (radius 30..330), the id map the discs painted in order: a third of the planes' rows are hit, as real instance
masks are mostly empty.  `--dense` fills every plane instead (every 64-pixel step is a hit: the kernel's slowest input).
One JSON with the commit hash is written to --out."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def discs(n, H, W, seed, dense):
    if dense:
        return torch.ones(n, H, W, dtype=torch.uint8)
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W]
    out = np.zeros((n, H, W), np.uint8)
    for i in range(n):
        r = g.integers(30, max(31, min(H, W) // 3))
        cy, cx = g.integers(0, H), g.integers(0, W)
        out[i] = (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    return torch.from_numpy(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--planes", type=int, default=100)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--dense", action="store_true")
    ap.add_argument("--commit", default=None, help="commit hash to record (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mask_boxes_bench.json"))
    args = ap.parse_args()
    from psalm_amd import hip_ops as H
    o = H.get_ops()
    n, S = args.planes, args.size
    big = discs(n, S, S, 1, args.dense).cuda().float()
    small = discs(3, 480, 854, 2, args.dense).cuda()
    lab = torch.zeros(S, S, dtype=torch.int32)
    for i, m in enumerate(discs(min(n, 100), S, S, 3, args.dense)):
        lab[m != 0] = i + 1
    lab = lab.cuda()
    bg_out = torch.empty_like(big)

    def binarize():
        rc = o.lib.psalm_binarize_gather(o._p(big), o._p(None), o._p(None), o._p(bg_out), n, ctypes.c_long(S * S), o._stream())
        o._check(rc, "psalm_binarize_gather")

    ob, oa = o.empty(n, 4), o.empty(n, dtype=torch.int32)
    sb, sa = o.empty(3, 4), o.empty(3, dtype=torch.int32)
    tab = o.empty(256, 5, dtype=torch.int32)
    cases = {"mask_boxes_f32": (lambda: o.mask_boxes(big, out_boxes=ob, out_areas=oa), big.numel() * 4, list(big.shape)),
             "binarize_gather": (binarize, big.numel() * 4, list(big.shape)),
             "mask_boxes_u8": (lambda: o.mask_boxes(small, out_boxes=sb, out_areas=sa), small.numel(), list(small.shape)),
             "label_boxes_i32": (lambda: o.label_boxes(lab, 256, out=tab), lab.numel() * 4, list(lab.shape))}
    # the results the timed calls produce are right (numpy on the same inputs), before anything is timed
    ys, xs = np.nonzero(small[1].cpu().numpy())
    o.mask_boxes(small, out_boxes=sb, out_areas=sa)
    assert sb[1].tolist() == [xs.min(), ys.min(), xs.max() + 1, ys.max() + 1] and int(sa[1]) == len(ys)
    o.mask_boxes(big, out_boxes=ob, out_areas=oa)
    assert torch.equal(oa.cpu(), big.sum((1, 2)).to(torch.int32).cpu())
    o.label_boxes(lab, 256, out=tab)
    assert torch.equal(tab[:, 4].cpu(), torch.bincount(lab.reshape(-1).cpu(), minlength=256)[:256].to(torch.int32))
    us = {k: [] for k in cases}
    for rep in range(args.reps + args.warmup):
        for name, (fn, _, _) in cases.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.inner):
                fn()
            e1.record()
            e1.synchronize()
            if rep >= args.warmup:
                us[name].append(e0.elapsed_time(e1) * 1e3 / args.inner)
    commit = args.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    res = {"commit": commit, "device": torch.cuda.get_device_name(0), "reps": args.reps, "inner": args.inner, "warmup": args.warmup,
           "input": "dense" if args.dense else "one disc per plane",
           "timing": "device events around `inner` back-to-back calls / inner, cases alternating; medians"}
    for name, (_, nbytes, shape) in cases.items():
        med = statistics.median(us[name])
        res[name] = {"shape": shape, "bytes_read": nbytes, "us_median": round(med, 2), "us_min": round(min(us[name]), 2),
                     "us_max": round(max(us[name]), 2), "read_GBps": round(nbytes / med * 1e-3, 1)}
    res["mask_boxes_f32_over_binarize_gather_per_byte_read"] = round(res["mask_boxes_f32"]["us_median"] / res["binarize_gather"]["us_median"], 3)
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
