"""Distance maps, centres and DAVIS's boundary F on the device -- evalout.mask_distance / mask_centers / boundary_counts -- against the host path
they replace: `masks.cpu()`, then scipy.ndimage.distance_transform_edt plane by plane (for F: the seg2bmap rules of tests/distance_util.py in
numpy, then the same transform of the boundary maps).

    python tools/bench_mask_distance.py [--reps 3] [--warmup 1] [--step-timeout 900] [--out profiles/mask_distance_bench.json]

Every case runs in a child process of its own under `--step-timeout` seconds (this process never opens the device); the first case that fails or
runs out of time ends the run with its exit status, and no case is started after it.
  distance_64     64 uint8 masks of 1024 x 1024 on the device: one disc or box each of mixed sizes, plane 0 a disc that fills most of the plane.
                  device = evalout.mask_distance (the inside map, border=False); host = `masks.cpu().numpy()` (64 MB over the bus) +
                  rint(distance_transform_edt(plane) ** 2).
  centers_64      the same masks: evalout.mask_centers; host = the copy + the transform of the plane padded with zeros + the first arg-max.
  boundary_f_64   64 pairs (mask k, mask k shifted by (3, 5)), bound 12: evalout.boundary_counts; host = both copies (128 MB) + seg2bmap and
                  the transform of every boundary map + the four sums.
Host clock around the call, device synchronised; the two agree on every output before anything is timed.  Medians of --reps samples after
--warmup, alternating.  One JSON with the commit hash is written to --out."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
CASES = ("distance_64", "centers_64", "boundary_f_64")
S, N, BOUND, SHIFT = 1024, 64, 12, (3, 5)


def workload():
    from bench_segment_everything import scene
    planes = scene(S, N, N, 2)[0]
    yy, xx = np.mgrid[:S, :S]
    planes[0] = (yy - S // 2) ** 2 + (xx - S // 2) ** 2 <= (S // 2 - 30) ** 2      # fills most of the plane: distances of several hundred
    return planes


def host_dist2(flags):
    from scipy import ndimage
    return np.rint(ndimage.distance_transform_edt(flags) ** 2).astype(np.int32)


def host_center(flags):
    if not flags.any():
        return [-1, -1, 0]
    d = host_dist2(np.pad(flags, 1))[1:-1, 1:-1]
    p = int(np.argmax(d))
    return [p // flags.shape[1], p % flags.shape[1], int(d.reshape(-1)[p])]


def host_counts(pred, gt, bound):
    from distance_util import np_bmap
    bp, bg = np_bmap(pred), np_bmap(gt)
    near_g = host_dist2(~bg) <= bound * bound if bg.any() else np.zeros_like(bg)
    near_p = host_dist2(~bp) <= bound * bound if bp.any() else np.zeros_like(bp)
    return [int(bp.sum()), int(bg.sum()), int((bp & near_g).sum()), int((bg & near_p).sum())]


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


def run_case(name, args):
    from psalm_amd import evalout as E
    from psalm_amd import hip_ops as H
    o = H.get_ops()
    planes = workload()
    dev = torch.from_numpy(planes).cuda()
    bus = N * S * S
    extra = {}
    if name == "distance_64":
        def device():
            return E.mask_distance(dev, ops=o)

        def host():
            return np.stack([host_dist2(p != 0) for p in dev.cpu().numpy()])

        got, want = device().cpu().numpy(), host()
        assert np.array_equal(got, want), "mask_distance and the host path disagree"
        extra = {"largest_distance": round(float(np.sqrt(got.max())), 1), "bytes_result_device_path": 4 * bus}
    elif name == "centers_64":
        def device():
            return E.mask_centers(dev, ops=o)

        def host():
            return [host_center(p != 0) for p in dev.cpu().numpy()]

        got, want = device().cpu().tolist(), host()
        assert got == want, "mask_centers and the host path disagree"
        extra = {"deepest_center": max(got, key=lambda c: c[2])}
    else:
        gt = torch.from_numpy(np.roll(planes, SHIFT, axis=(1, 2))).cuda()
        pairs = [(k, k) for k in range(N)]
        bus *= 2

        def device():
            return E.boundary_counts(dev, gt, pairs, BOUND, ops=o)

        def host():
            p, g = dev.cpu().numpy(), gt.cpu().numpy()
            return [host_counts(p[a] != 0, g[b] != 0, BOUND) for a, b in pairs]

        got, want = device(), host()
        assert got.cpu().tolist() == want, "boundary_counts and the host path disagree"
        extra = {"pairs": N, "bound": BOUND, "shift": list(SHIFT), "mean_F": round(float(E.boundary_f(got)[2].mean()), 4)}
    res = {"device_name": torch.cuda.get_device_name(0), "masks": [N, S, S], "dtype": "uint8", "host_transform": "scipy.ndimage.distance_transform_edt",
           "bytes_over_the_bus_host_path": bus, "timing": "host clock around the call, device synchronised; medians, the two alternating"}
    res.update(extra)
    res.update(timed((("device", device), ("host", host)), args))
    res["host_over_device"] = round(res["host_ms_median"] / res["device_ms_median"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--step-timeout", type=int, default=900)
    ap.add_argument("--case", default=None, help="(internal) run one case in this process and print its JSON")
    ap.add_argument("--commit", default=None, help="commit hash to record (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mask_distance_bench.json"))
    args = ap.parse_args()
    if args.case:
        print("RESULT " + json.dumps(run_case(args.case, args)), flush=True)
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
