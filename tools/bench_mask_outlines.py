"""Mask outlines on the device -- evalout.mask_outlines, PSALM.segment_everything(outlines=True) -- against the cheapest first step of any host
tracer: the device-to-pinned-host copy of the same uint8 planes, measured in the same run.

    python tools/bench_mask_outlines.py [--reps 5] [--warmup 1] [--step-timeout 600] [--out profiles/mask_outlines_bench.json]

Every case runs in a child process of its own under `--step-timeout` seconds (this process never opens the device); the first case that fails or
runs out of time ends the run with its exit status, and no case is started after it.
  outlines_noisy_64  64 uint8 masks of 1024 x 1024 on the device: overlapping discs, 2 % of the pixels flipped (salt noise: tens of thousands of
                     one-pixel rings per plane).  device = evalout.mask_outlines(connectivity=8), host clock around the call, device
                     synchronised; copy = the same planes into a pinned host buffer (64 MB over the bus), host clock, synchronised.  Before
                     anything is timed: filling the outlines gives the planes back, the areas add up to mask_boxes' and the outer rings to
                     mask_components' counts.  Medians of --reps samples after --warmup, alternating.
  outlines_clean_64  the same masks after evalout.clean_masks(min_island=16, max_hole=16): a few rings per plane, what a click-to-mask tool outlines.
  everything_R64     the scene of tools/bench_segment_everything.py (24 objects, an 8 x 8 grid of clicks, 100 float32 query planes):
                     PSALM._everything_dedup without and with outlines=True; host clock around the call, device synchronised.
One JSON with the commit hash is written to --out."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
CASES = ("outlines_noisy_64", "outlines_clean_64", "everything_R64")
MIN_ISLAND, MAX_HOLE, CONN = 16, 16, 8


def noisy_discs(n, S, seed, flip=0.02):
    """n planes with one random disc each (neighbours overlap a lot), `flip` of the pixels inverted"""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[:S, :S]
    out = np.zeros((n, S, S), np.uint8)
    for i in range(n):
        cy, cx, r = g.integers(S // 4, 3 * S // 4), g.integers(S // 4, 3 * S // 4), g.integers(S // 8, S // 3)
        out[i][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 1
        out[i] ^= (g.random((S, S)) < flip).astype(np.uint8)
    return out


def timed(fns, args):
    ms = {k: [] for k, _ in fns}
    for rep in range(args.reps + args.warmup):
        for k, fn in fns:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep >= args.warmup:
                ms[k].append((time.perf_counter() - t0) * 1e3)
    res = {}
    for k in ms:
        res[k + "_ms_median"], res[k + "_ms_min"], res[k + "_ms_max"] = (round(f(ms[k]), 3) for f in (statistics.median, min, max))
    return res


def run_planes(name, args):
    from psalm_amd import evalout as E
    from psalm_amd import hip_ops as H
    o = H.get_ops()
    S, n = 1024, 64
    dev = torch.from_numpy(noisy_discs(n, S, 7)).cuda()
    if name == "outlines_clean_64":
        dev = E.clean_masks(dev, min_island=MIN_ISLAND, max_hole=MAX_HOLE, connectivity=CONN, ops=o)["masks"]
    pinned = torch.empty((n, S, S), dtype=torch.uint8).pin_memory()

    def device():
        return E.mask_outlines(dev, connectivity=CONN, ops=o)

    def copy():
        pinned.copy_(dev, non_blocking=True)

    got = device()
    assert torch.equal(E.fill_polygons(got["rings"], got["vertices"], dev.shape, ops=o), dev), "filling the outlines does not give the masks back"
    rings = got["rings"].cpu().numpy()
    area = np.bincount(rings[:, 0], weights=rings[:, 3], minlength=n).astype(np.int64)
    assert area.tolist() == o.mask_boxes(dev)[1].cpu().tolist(), "the ring areas do not add up to the masks' pixels"
    outer = np.bincount(rings[rings[:, 3] > 0, 0], minlength=n)
    assert outer.tolist() == o.mask_components(dev, connectivity=CONN, want_table=False)[1].cpu().tolist(), "outer rings and components disagree"
    res = {"device_name": torch.cuda.get_device_name(0), "masks": [n, S, S], "dtype": "uint8", "connectivity": CONN,
           "rings_total": int(rings.shape[0]), "vertices_total": int(got["vertices"].shape[0]), "bytes_over_the_bus_copy": n * S * S,
           "bytes_of_the_result": int(rings.nbytes + got["vertices"].numel() * 4 + 8 * n),
           "timing": "host clock around the call, device synchronised; medians, the two alternating"}
    if name == "outlines_clean_64":
        res.update(min_island=MIN_ISLAND, max_hole=MAX_HOLE)
    res.update(timed((("device", device), ("copy", copy)), args))
    res["device_over_copy"] = round(res["device_ms_median"] / res["copy_ms_median"], 2)
    return res


def run_everything(name, args):
    from bench_segment_everything import DEN, NUM, scene
    from psalm_amd import hip_ops as H
    from psalm_amd.session import SessionMixin
    o = H.get_ops()
    S, Q, n_obj, gy, gx = 1024, 100, 24, 8, 8
    R = gy * gx
    planes, obj_scores = scene(S, n_obj, Q, 1)
    query, score = [], []
    for i in range(gy):
        for j in range(gx):
            y, x = (2 * i + 1) * S // (2 * gy), (2 * j + 1) * S // (2 * gx)
            hit = [q for q in range(n_obj) if planes[q, y, x]]
            best = max(hit, key=lambda q: obj_scores[q]) if hit else n_obj
            query.append(best)
            score.append(obj_scores[best] if hit else 0.0)
    pred = torch.from_numpy(planes).cuda().float()
    q32 = torch.tensor(query, dtype=torch.int32, device="cuda")
    prompt = {"instances": types.SimpleNamespace(pred_masks=pred), "picked_query": q32.to(torch.int64),
              "picked_scores": torch.tensor(score, dtype=torch.float32, device="cuda")}
    me = types.SimpleNamespace(ops=o)

    def plain():
        return SessionMixin._everything_dedup(me, [prompt], (R,), NUM, DEN, 1, None)

    def outlined():
        return SessionMixin._everything_dedup(me, [prompt], (R,), NUM, DEN, 1, None, outlines=True)

    a, b = plain(), outlined()
    assert torch.equal(a["masks"], b["masks"]) and torch.equal(a["labels"], b["labels"])
    from psalm_amd import evalout as E
    back = E.fill_polygons(b["outlines"]["rings"], b["outlines"]["vertices"], b["masks"].shape, ops=o)
    assert torch.equal(back, b["masks"]), "filling the survivors' outlines does not give their masks back"
    res = {"device_name": torch.cuda.get_device_name(0), "image": [S, S], "grid": [gy, gx], "R": R, "query_planes": Q, "objects": n_obj,
           "kept": int(a["masks"].shape[0]), "rings_total": int(b["outlines"]["rings"].shape[0]),
           "vertices_total": int(b["outlines"]["vertices"].shape[0]),
           "timing": "host clock around the call, device synchronised; medians, the two alternating"}
    res.update(timed((("plain", plain), ("outlines", outlined)), args))
    res["outlines_over_plain"] = round(res["outlines_ms_median"] / res["plain_ms_median"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--step-timeout", type=int, default=600)
    ap.add_argument("--case", default=None, help="(internal) run one case in this process and print its JSON")
    ap.add_argument("--commit", default=None, help="commit hash to record (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mask_outlines_bench.json"))
    args = ap.parse_args()
    if args.case:
        fn = run_everything if args.case.startswith("everything") else run_planes
        print("RESULT " + json.dumps(fn(args.case, args)), flush=True)
        return 0
    commit = args.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    res = {"commit": commit, "reps": args.reps, "warmup": args.warmup}
    for name in CASES:
        cmd = [sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(args.reps), "--warmup", str(args.warmup)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            print(f"{name}: no result within {args.step_timeout} s; stopping", file=sys.stderr)
            return 124
        line = next((ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")), None)
        if r.returncode or line is None:
            print(f"{name}: exit status {r.returncode}; stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
            return r.returncode or 1
        res[name] = json.loads(line[7:])
        print(name, json.dumps(res[name]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
