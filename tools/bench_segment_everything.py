"""The device step of PSALM.segment_everything -- pack into bit planes, all-pairs intersections, greedy NMS, label map, ONE read-back, unpack and
boxes of the survivors -- against the host path it replaces: `picked_masks.cpu()`, a numpy IoU matrix, greedy NMS in Python.

    python tools/bench_segment_everything.py [--reps 20] [--warmup 3] [--step-timeout 300] [--out profiles/segment_everything_bench.json]

Every case runs in a child process of its own under `--step-timeout` seconds (this process never opens the device); the first case that fails or
runs out of time ends the run with its exit status, and no case is started after it.
  everything_R64 / everything_R192   a 1024 x 1024 image with 24 objects (discs and boxes), an 8 x 8 / 12 x 16 grid of clicks; every click picks,
                     among 100 float32 query planes (419 MB), the object under it (or an empty plane) with that object's score: what
                     `segment(..., pick=True)` leaves on the device.  device = PSALM._everything_dedup on it, host clock around the call (it ends in
                     its read-back and the survivors' unpack + boxes, then a device synchronise); host = `picked_masks.cpu()` + numpy + Python NMS
                     under the same integer rule, host clock.  The two agree on the kept list before anything is timed.  Medians of --reps
                     samples after --warmup, the two alternating sample by sample.
  pairs_m64 / pairs_m256 / pairs_m1024   psalm_mask_pair_counts alone on random bit planes of 1024 x 1024 pixels (nw = 16384 words), a against
                     itself: device events around `--inner` back-to-back calls / inner (the memset node included).  word_pairs/s = m^2 nw / time
                     (one 64-bit and + popcount + add each); operand bytes = m nw 8.
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
CASES = ("everything_R64", "everything_R192", "pairs_m64", "pairs_m256", "pairs_m1024")
GRIDS = {"everything_R64": (8, 8), "everything_R192": (12, 16)}
NUM, DEN = 7, 10


def scene(S, n_obj, Q, seed):
    """(planes (Q, S, S) uint8: the first n_obj hold one disc or box each, the rest are empty; scores (n_obj))"""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[:S, :S]
    out = np.zeros((Q, S, S), np.uint8)
    for i in range(n_obj):
        cy, cx, r = g.integers(0, S), g.integers(0, S), g.integers(S // 16, S // 5)
        if i % 2:
            out[i] = (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
        else:
            out[i, max(0, cy - r): cy + r, max(0, cx - r // 2): cx + r // 2] = 1
    return out, g.random(n_obj).astype(np.float32)


def host_nms(pm_host, scores):
    """the path a caller has today, on the R masks it pulled across the bus: IoU counts with one BLAS product (exact: counts < 2^24), greedy NMS"""
    R = pm_host.shape[0]
    flags = (pm_host.reshape(R, -1) != 0).astype(np.float32)
    inter = (flags @ flags.T).astype(np.int64)
    areas = np.diag(inter)
    kept = []
    for i in sorted(range(R), key=lambda i: (-float(scores[i]), i)):
        if areas[i] < 1:
            continue
        if not any(DEN * inter[i, j] > NUM * (areas[i] + areas[j] - inter[i, j]) for j in kept):
            kept.append(i)
    return kept


def run_everything(name, args):
    from psalm_amd import hip_ops as H
    from psalm_amd.session import SessionMixin
    o = H.get_ops()
    S, Q, n_obj = 1024, 100, 24
    gy, gx = GRIDS[name]
    R = gy * gx
    planes, obj_scores = scene(S, n_obj, Q, 1)
    query, score = [], []
    for i in range(gy):
        for j in range(gx):
            y, x = (2 * i + 1) * S // (2 * gy), (2 * j + 1) * S // (2 * gx)
            hit = [q for q in range(n_obj) if planes[q, y, x]]
            best = max(hit, key=lambda q: obj_scores[q]) if hit else n_obj          # (plane n_obj is empty)
            query.append(best)
            score.append(obj_scores[best] if hit else 0.0)
    pred = torch.from_numpy(planes).cuda().float()
    q32 = torch.tensor(query, dtype=torch.int32, device="cuda")
    prompt = {"instances": types.SimpleNamespace(pred_masks=pred), "picked_query": q32.to(torch.int64),
              "picked_scores": torch.tensor(score, dtype=torch.float32, device="cuda"), "picked_masks": o.mask_gather_u8(pred, q32)}
    me = types.SimpleNamespace(ops=o)

    def device():
        out = SessionMixin._everything_dedup(me, [prompt], (R,), NUM, DEN, 1, None)
        torch.cuda.synchronize()
        return out

    def host():
        return host_nms(prompt["picked_masks"].cpu().numpy(), score)

    dev_out, kept = device(), host()
    assert dev_out["regions"].tolist() == kept, "the device step and the host path disagree"
    ms = {"device": [], "host": []}
    for rep in range(args.reps + args.warmup):
        for k, fn in (("device", device), ("host", host)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            if rep >= args.warmup:
                ms[k].append((time.perf_counter() - t0) * 1e3)
    res = {"device_name": torch.cuda.get_device_name(0), "image": [S, S], "grid": [gy, gx], "R": R, "query_planes": Q, "objects": n_obj, "kept": len(kept), "iou_thr": [NUM, DEN],
           "bytes_over_the_bus_host_path": R * S * S, "timing": "host clock around the call, device synchronised; medians, the two alternating"}
    for k in ms:
        res[k + "_ms_median"], res[k + "_ms_min"], res[k + "_ms_max"] = (round(f(ms[k]), 3) for f in (statistics.median, min, max))
    res["host_over_device"] = round(res["host_ms_median"] / res["device_ms_median"], 2)
    return res


def run_pairs(name, args):
    from psalm_amd import hip_ops as H
    o = H.get_ops()
    m, nw = int(name.split("_m")[1]), 1024 * 1024 // 64
    g = torch.Generator(device="cuda").manual_seed(m)
    bits = torch.randint(-2 ** 63, 2 ** 63 - 1, (m, nw), dtype=torch.int64, device="cuda", generator=g)
    inter = o.empty(m, m, dtype=torch.int32)
    o.mask_pair_counts(bits, out=inter)
    rows = np.unpackbits(bits[:3].cpu().numpy().view(np.uint8), axis=1).astype(np.int64)       # (the bit order inside a byte does not matter to a count)
    assert np.array_equal(inter[:3, :3].cpu().numpy(), rows @ rows.T), "psalm_mask_pair_counts disagrees with numpy"
    us = []
    for rep in range(args.reps + args.warmup):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.inner):
            o.mask_pair_counts(bits, out=inter)
        e1.record()
        e1.synchronize()
        if rep >= args.warmup:
            us.append(e0.elapsed_time(e1) * 1e3 / args.inner)
    med = statistics.median(us)
    return {"device_name": torch.cuda.get_device_name(0), "m": m, "nw": nw, "operand_bytes": m * nw * 8, "us_median": round(med, 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2),
            "word_pairs_per_s": round(m * m * nw / med * 1e6, 0), "timing": "device events around `inner` back-to-back calls / inner; median"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--case", default=None, help="(internal) run one case in this process and print its JSON")
    ap.add_argument("--commit", default=None, help="commit hash to record (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segment_everything_bench.json"))
    args = ap.parse_args()
    if args.case:
        fn = run_everything if args.case.startswith("everything") else run_pairs
        print("RESULT " + json.dumps(fn(args.case, args)), flush=True)
        return 0
    commit = args.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    res = {"commit": commit, "reps": args.reps, "inner": args.inner, "warmup": args.warmup}
    for name in CASES:
        cmd = [sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(args.reps), "--inner", str(args.inner), "--warmup", str(args.warmup)]
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
