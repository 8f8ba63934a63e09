"""Mask cleanup and connected components on the device -- evalout.clean_masks / mask_components, PSALM.segment_everything(min_island=, max_hole=)
-- against the host path they replace: `masks.cpu()`, then labelling plane by plane (scipy.ndimage.label where importable, else the numpy
oracle of tests/components_util.py).

    python tools/bench_mask_components.py [--reps 5] [--warmup 1] [--step-timeout 600] [--out profiles/mask_components_bench.json]

Every case runs in a child process of its own under `--step-timeout` seconds (this process never opens the device); the first case that fails or
runs out of time ends the run with its exit status, and no case is started after it.
  clean_64 / components_64   64 uint8 masks of 1024 x 1024 on the device: one disc or box each, 200 specks of 1 .. 3 pixels, 200 pin-holes.
                     device = evalout.clean_masks(min_island=16, max_hole=16) / evalout.mask_components(max_components=256), host clock around the
                     call, device synchronised; host = `masks.cpu().numpy()` (64 MB over the bus) + the same rules plane by plane, host clock.
                     The two agree on every output before anything is timed.  Medians of --reps samples after --warmup, alternating.
  everything_R64     the scene of tools/bench_segment_everything.py (24 objects, an 8 x 8 grid of clicks, 100 float32 query planes) with the same
                     specks and pin-holes in every object plane: PSALM._everything_dedup without cleaning -- launch for launch the parent
                     commit's device step -- and with min_island = max_hole = 16; host clock around the call, device synchronised.
One JSON with the commit hash is written to --out; `segment_everything_parent_record` quotes profiles/segment_everything_bench.json (the parent
commit's measurement of the device step without cleaning) when that file is there."""
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
CASES = ("clean_64", "components_64", "everything_R64")
MIN_ISLAND, MAX_HOLE, CONN = 16, 16, 8

try:
    from scipy import ndimage as _ndi
except Exception:                                                      # no scipy: the tests' oracle
    _ndi = None
    sys.path.insert(0, os.path.join(ROOT, "tests"))


def host_label(flags, conn):
    if _ndi is not None:
        return _ndi.label(flags, structure=np.ones((3, 3)) if conn == 8 else None)
    from components_util import np_components
    return np_components(flags, conn)


def host_clean(flags, min_island, max_hole, conn):
    """the rules of psalm_mask_clean on one host plane"""
    out = flags.copy()
    if max_hole > 0:
        lab, n = host_label(~out, 4 if conn == 8 else 8)
        area = np.bincount(lab.ravel(), minlength=n + 1)
        on_border = np.zeros(n + 1, bool)
        for edge in (lab[0], lab[-1], lab[:, 0], lab[:, -1]):
            on_border[edge] = True
        fill = ~on_border & (area <= max_hole)
        fill[0] = False
        out |= fill[lab]
    if min_island > 0:
        lab, n = host_label(out, conn)
        drop = np.bincount(lab.ravel(), minlength=n + 1) < min_island
        drop[0] = False
        out &= ~drop[lab]
    return out


def speckle(planes, seed, n=200):
    """n specks of 1 .. 3 pixels and n pin-holes of 1 .. 2 pixels in every non-empty plane, in place"""
    g = np.random.default_rng(seed)
    S = planes.shape[-1]
    for p in planes:
        if not p.any():
            continue
        ys, xs = np.nonzero(p[1:-1, 1:-2])
        pick = g.integers(0, len(ys), n)
        yy, xx = g.integers(1, S - 1, n), g.integers(1, S - 2, n)
        two, three = g.random(n) < 0.5, g.random(n) < 0.25
        p[yy, xx] = 1
        p[yy[two], xx[two] + 1] = 1
        p[yy[three] + 1, xx[three]] = 1
        p[ys[pick] + 1, xs[pick] + 1] = 0
        p[ys[pick][two] + 1, xs[pick][two] + 2] = 0
    return planes


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
    from bench_segment_everything import scene
    from psalm_amd import evalout as E
    from psalm_amd import hip_ops as H
    o = H.get_ops()
    S, n = 1024, 64
    planes = speckle(scene(S, n, n, 2)[0], 3)
    dev = torch.from_numpy(planes).cuda()
    if name == "clean_64":
        def device():
            return E.clean_masks(dev, min_island=MIN_ISLAND, max_hole=MAX_HOLE, connectivity=CONN, ops=o)

        def host():
            return np.stack([host_clean(p != 0, MIN_ISLAND, MAX_HOLE, CONN) for p in dev.cpu().numpy()])

        got, want = device(), host()
        assert np.array_equal(got["masks"].cpu().numpy() != 0, want), "clean_masks and the host path disagree"
        assert got["areas"].cpu().tolist() == want.reshape(n, -1).sum(1).tolist()
        extra = {"removed_pixels": int(got["removed"].sum()), "filled_pixels": int(got["filled"].sum())}
    else:
        def device():
            return E.mask_components(dev, connectivity=CONN, max_components=256, ops=o)

        def host():
            return [host_label(p != 0, CONN) for p in dev.cpu().numpy()]

        got, want = device(), host()
        assert got["count"].cpu().tolist() == [int(c) for _, c in want], "mask_components and the host path disagree on the counts"
        assert np.array_equal(got["labels"].cpu().numpy(), np.stack([l for l, _ in want])), "mask_components and the host path disagree"
        extra = {"components_total": int(got["count"].sum())}
    res = {"device_name": torch.cuda.get_device_name(0), "masks": [n, S, S], "dtype": "uint8", "connectivity": CONN,
           "host_labelling": "scipy.ndimage.label" if _ndi is not None else "tests/components_util.py", "bytes_over_the_bus_host_path": n * S * S,
           "timing": "host clock around the call, device synchronised; medians, the two alternating"}
    if name == "clean_64":
        res.update(min_island=MIN_ISLAND, max_hole=MAX_HOLE)
    res.update(extra)
    res.update(timed((("device", device), ("host", host)), args))
    res["host_over_device"] = round(res["host_ms_median"] / res["device_ms_median"], 2)
    return res


def run_everything(name, args):
    from bench_segment_everything import DEN, NUM, scene
    from psalm_amd import hip_ops as H
    from psalm_amd.session import SessionMixin
    o = H.get_ops()
    S, Q, n_obj, gy, gx = 1024, 100, 24, 8, 8
    R = gy * gx
    planes, obj_scores = scene(S, n_obj, Q, 1)
    clean_planes = planes.copy()
    speckle(planes, 3)
    query, score = [], []
    for i in range(gy):
        for j in range(gx):
            y, x = (2 * i + 1) * S // (2 * gy), (2 * j + 1) * S // (2 * gx)
            hit = [q for q in range(n_obj) if clean_planes[q, y, x]]
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

    def cleaning():
        return SessionMixin._everything_dedup(me, [prompt], (R,), NUM, DEN, 1, None, MIN_ISLAND, MAX_HOLE, CONN)

    a, b = plain(), cleaning()
    want = np.stack([host_clean(planes[q] != 0, MIN_ISLAND, MAX_HOLE, CONN) for q in np.asarray(query)[b["regions"].cpu().numpy()]])
    assert np.array_equal(b["masks"].cpu().numpy() != 0, want), "the cleaned survivors and the host path disagree"
    res = {"device_name": torch.cuda.get_device_name(0), "image": [S, S], "grid": [gy, gx], "R": R, "query_planes": Q, "objects": n_obj,
           "kept_plain": int(a["masks"].shape[0]), "kept_cleaning": int(b["masks"].shape[0]), "min_island": MIN_ISLAND, "max_hole": MAX_HOLE,
           "removed_pixels": int(b["cleaned"][:, 0].sum()), "filled_pixels": int(b["cleaned"][:, 1].sum()),
           "timing": "host clock around the call, device synchronised; medians, the two alternating"}
    res.update(timed((("plain", plain), ("cleaning", cleaning)), args))
    res["cleaning_over_plain"] = round(res["cleaning_ms_median"] / res["plain_ms_median"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--step-timeout", type=int, default=600)
    ap.add_argument("--case", default=None, help="(internal) run one case in this process and print its JSON")
    ap.add_argument("--commit", default=None, help="commit hash to record (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mask_components_bench.json"))
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
    parent = os.path.join(ROOT, "profiles", "segment_everything_bench.json")
    if os.path.exists(parent):
        with open(parent) as fh:
            rec = json.load(fh)
        res["segment_everything_parent_record"] = {"commit": rec.get("commit"), "everything_R64": rec.get("everything_R64")}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
