"""Panoptic quality on the device -- evalout.PanopticQuality.update -- against the host path it replaces: `.cpu()` of the two id maps, then the
numpy restatement of panopticapi's pq_compute_single_core (tests/panoptic_quality_util.py: np.unique over gt * 256^3 + pred and the match in
dicts).  The PNG encode / decode and the JSON file of the reference's evaluator are NOT in the host figure: it is the floor of that path.

    python tools/bench_panoptic_quality.py [--reps 20] [--warmup 3] [--step-timeout 600] [--out profiles/panoptic_quality_bench.json]

Every case runs in a child process of its own under `--step-timeout` seconds (this process never opens the device); the first case that fails or
runs out of time ends the run with its exit status, and no case is started after it.
  coco_like_1024   a 1024 x 1024 prediction of 100 segments (Voronoi regions) against a ground truth of about 40 segments with two crowd regions
                   and a VOID region, both int32 on the device.  device = PanopticQuality.update (one small upload, psalm_label_pair_counts,
                   psalm_pq_accumulate, no read-back; the device is synchronised for the clock); host = both maps `.cpu().numpy()` (8 MB over the
                   bus) + pq_single.
  coco_like_1024_rgb_gt   the same with the ground truth as the PNG's (H,W,3) uint8 array on the device.
Host clock around the call, device synchronised; the accumulators of the two agree (integers equal, IoU sums bit for bit) before anything is timed.
Medians of --reps samples after --warmup, alternating.  One JSON with the commit hash is written to --out."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
CASES = ("coco_like_1024", "coco_like_1024_rgb_gt")
S, N_PRED, N_GT = 1024, 100, 40
CATEGORIES = {c: c <= 80 for c in range(1, 134)}               # 80 things, 53 stuff


def regions(ys, xs):
    """(S,S) index of the nearest site (a running minimum: no (S,S,n) block)"""
    yy, xx = np.mgrid[:S, :S]
    best, arg = np.full((S, S), np.iinfo(np.int64).max), np.zeros((S, S), np.int64)
    for k, (y, x) in enumerate(zip(ys.tolist(), xs.tolist())):
        d = (yy - y) ** 2 + (xx - x) ** 2
        arg[d < best] = k
        best = np.minimum(best, d)
    return arg


def workload():
    """(scene, categories): ground truth = the Voronoi regions of 41 sites, region 0 VOID, two of them crowd; prediction = the regions of those
    sites moved a little plus 59 more, so that many predicted segments are a ground-truth segment with a piece missing; ids as a COCO PNG's"""
    import panoptic_quality_util as U
    rng = np.random.default_rng(7)
    ys, xs = rng.integers(0, S, N_GT + 1), rng.integers(0, S, N_GT + 1)
    g_reg = regions(ys, xs)
    g_ids = rng.choice(np.arange(1000, 2 ** 24 - 1), N_GT + 1, replace=False)
    g_cat = rng.integers(1, 134, N_GT + 1)
    gt = g_ids[g_reg]
    gt[g_reg == 0] = 0
    gt_info = [{"id": int(g_ids[k]), "category_id": int(g_cat[k]), "iscrowd": int(k in (1, 2))} for k in range(1, N_GT + 1)]
    more = N_PRED - (N_GT + 1)
    p_reg = regions(np.concatenate((np.clip(ys + rng.integers(-6, 7, N_GT + 1), 0, S - 1), rng.integers(0, S, more))),
                    np.concatenate((np.clip(xs + rng.integers(-6, 7, N_GT + 1), 0, S - 1), rng.integers(0, S, more))))
    pred = 1 + p_reg
    owner = [int(np.bincount(g_reg[p_reg == k], minlength=N_GT + 1).argmax()) if (p_reg == k).any() else 0 for k in range(N_PRED)]
    pred_info = [{"id": k + 1, "category_id": int(g_cat[owner[k]] if rng.random() < 0.85 else rng.integers(1, 134))} for k in range(N_PRED)]
    return U.scene(gt, gt_info, pred, pred_info), CATEGORIES


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
    import panoptic_quality_util as U
    from psalm_amd import evalout as E
    from psalm_amd import hip_ops as H
    o = H.get_ops()
    sc, cats = workload()
    rgb = name.endswith("_rgb_gt")
    pred = torch.from_numpy(sc["pred"]).cuda()
    gt = torch.from_numpy(U.np_id2rgb(sc["gt"]) if rgb else sc["gt"]).cuda()
    meter = E.PanopticQuality(cats, ops=o)
    stat, notes = U.new_stat(cats)

    def device():
        meter.update(pred, sc["pred_info"], gt, sc["gt_info"])

    def host():
        U.pq_single(stat, notes, gt.cpu().numpy(), sc["gt_info"], pred.cpu().numpy(), sc["pred_info"])

    device()
    host()
    s, i, n = U.stat_arrays(stat, notes, cats)
    assert np.array_equal(meter.stat.cpu().numpy(), s) and np.array_equal(meter.notes.cpu().numpy(), n), "the device meter and the host path disagree"
    assert np.array_equal(meter.iou.cpu().numpy().view(np.int64), i.view(np.int64)), "the IoU sums of the device meter and the host path differ"
    first = meter.results(strict=False)
    res = {"device_name": torch.cuda.get_device_name(0), "map": [S, S], "gt_form": "rgb uint8" if rgb else "int32", "pred_segments": len(sc["pred_info"]),
           "gt_segments": len(sc["gt_info"]), "gt_crowd_segments": sum(g["iscrowd"] for g in sc["gt_info"]),
           "tp_fp_fn_of_one_image": [int(v) for v in s.sum(0)], "pq_of_one_image": round(first["All"]["pq"], 4),
           "bytes_over_the_bus_host_path": int(gt.numel() * gt.element_size() + pred.numel() * 4),
           "host_path": "maps .cpu().numpy() + numpy restatement of panopticapi pq_compute_single_core (no PNG, no JSON)",
           "timing": "host clock around the call, device synchronised; medians, the two alternating"}
    res.update(timed((("device", device), ("host", host)), args))
    res["host_over_device"] = round(res["host_ms_median"] / res["device_ms_median"], 2)
    lib = o.lib                                                  # the two launches alone, between events
    lib.records = []
    try:
        device()
        torch.cuda.synchronize()
        res["launch_ms"] = {r[0]: round(r[2].elapsed_time(r[3]), 4) for r in lib.records}
    finally:
        lib.records = None
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=600)
    ap.add_argument("--case", default=None, help="(internal) run one case in this process and print its JSON")
    ap.add_argument("--commit", default=None, help="commit hash to record (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "panoptic_quality_bench.json"))
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
