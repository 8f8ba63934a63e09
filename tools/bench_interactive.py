"""Interactive image sessions: what does one click cost as `segment(regions=...)` (prompt prepared on the device) against the host preparation of the
dataset mapper + `segment(seg_info=...)`, on the same session in the same process?

    python tools/bench_interactive.py [--clicks 20] [--warmup 3] [--layers 24] [--out profiles/interactive_bench.json]

Full synthetic region model, precision "f16x3", a 1024^2 canvas.  For originals of 480 x 640 and 1024 x 1024, 1 and 3 regions per prompt, point and
scribble prompts:
  (a) `segment(sess, ids, am, regions=[G])`;
  (b) the host way: draw the prompt into an (h, w) mask, enhance_with_circles, apply_segmentation, wrap it as `instances.region_masks`,
      `segment(sess, ids, am, seg_info=[info])` -- and the host preparation alone (b0).
Every click lands somewhere else (the same sequence on both sides).  Each figure: wall time of a synchronous call, median of `--clicks` clicks after
`--warmup`.  The claim under test: (b) - (a) is about (b0).  One JSON with the commit hash is written to --out.
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


def timed(fn, clicks, warmup):
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    wall = []
    for i in range(clicks):
        t = time.perf_counter()
        fn(warmup + i)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t) * 1e3)
    return {"ms_median": round(statistics.median(wall), 3), "ms_min": round(min(wall), 3), "ms_max": round(max(wall), 3), "clicks": clicks}


def stroke(rng, h, w, n=300):
    """a scribble of about n pixels: a straight stroke between two random points"""
    (y0, y1), (x0, x1) = rng.integers(0, h, 2), rng.integers(0, w, 2)
    t = np.linspace(0.0, 1.0, n)
    return sorted(set(zip(np.round(y0 + (y1 - y0) * t).astype(int).tolist(), np.round(x0 + (x1 - x0) * t).astype(int).tolist())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clicks", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--originals", nargs="+", default=["480x640", "1024x1024"])
    ap.add_argument("--regions", type=int, nargs="+", default=[1, 3])
    ap.add_argument("--kinds", nargs="+", default=["points", "scribble"])
    ap.add_argument("--commit", default=None, help="commit hash to record (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "interactive_bench.json"))
    args = ap.parse_args()
    if args.clicks < 20 or args.warmup < 3:
        ap.error("the figures are medians of at least 20 clicks after at least 3 warm-ups")
    from psalm_amd.config import IMAGE_TOKEN_INDEX, REGION_TOKEN_INDEX, SEG_TOKEN_INDEX, PsalmConfig
    from psalm_amd.model import PSALM
    from psalm_amd.preprocess import apply_segmentation, enhance_with_circles
    from psalm_amd.synthetic import RegionInstances, make_state_dict, resized_box
    commit = args.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    S = args.size
    cfg = PsalmConfig(num_layers=args.layers, seg_task="region")
    model = PSALM(cfg, make_state_dict(cfg, seed=1), precision="f16x3", use_graphs=False)
    res = {"commit": commit, "device": torch.cuda.get_device_name(0), "precision": "f16x3", "layers": args.layers, "canvas": S, "cases": []}
    g = torch.Generator().manual_seed(7)
    n_draws = args.clicks + args.warmup
    for orig in args.originals:
        h, w = [int(v) for v in orig.split("x")]
        nh, nw = resized_box(h, w, S)
        tr = {"resize": (h, w, nh, nw), "pad": (S - nh, S - nw)}
        img = torch.randn(1, 3, S, S, generator=g)
        img[:, :, nh:, :] = 0
        img[:, :, :, nw:] = 0
        pm = torch.zeros(S, S, dtype=torch.bool)
        pm[nh:, :] = True
        pm[:, nw:] = True
        info = {"padding_mask": pm, "height": h, "width": w, "transforms": tr}
        sess = model.encode_image(img.cuda(), info)
        for k in args.regions:
            ids = torch.randint(5, cfg.vocab_size, (3,), generator=g).tolist() + [IMAGE_TOKEN_INDEX] + torch.randint(5, cfg.vocab_size, (2,), generator=g).tolist() \
                + [REGION_TOKEN_INDEX] * k + torch.randint(5, cfg.vocab_size, (2,), generator=g).tolist() + [SEG_TOKEN_INDEX] + [7]
            ids = torch.tensor([ids], dtype=torch.int64)
            am = torch.ones_like(ids, dtype=torch.bool)
            gt = torch.zeros(k, S, S)
            for kind in args.kinds:
                rng = np.random.default_rng(h * 7 + k)
                if kind == "points":
                    draws = [[{"points": [(int(rng.integers(0, h)), int(rng.integers(0, w)))]} for _ in range(k)] for _ in range(n_draws)]
                else:
                    draws = [[{"scribble": stroke(rng, h, w)} for _ in range(k)] for _ in range(n_draws)]
                radius = 10 if kind == "points" else 5

                def prepare(i):
                    masks = []
                    for rp in draws[i]:
                        m = np.zeros((h, w), np.uint8)
                        ys, xs = zip(*rp[kind])
                        m[list(ys), list(xs)] = 1
                        masks.append(apply_segmentation(enhance_with_circles(m, radius), tr))
                    return dict(info, instances=RegionInstances(torch.from_numpy(np.stack(masks)), gt))

                def host(i):
                    torch.manual_seed(i)
                    return model.segment(sess, ids, am, seg_info=[prepare(i)])

                def device(i):
                    torch.manual_seed(i)
                    return model.segment(sess, ids, am, regions=[draws[i]])

                a, b = device(0)[0], host(0)[0]                  # the two ways give the same answer (same RNG state, same draws)
                assert torch.equal(a["mask_pred"], b["mask_pred"]) and torch.equal(a["instances"].scores, b["instances"].scores)
                row = {"original": [h, w], "regions": k, "prompt": kind,
                       "segment_regions": timed(device, args.clicks, args.warmup),
                       "host_prepare_plus_segment": timed(host, args.clicks, args.warmup),
                       "host_prepare": timed(prepare, args.clicks, args.warmup)}
                row["saved_ms"] = round(row["host_prepare_plus_segment"]["ms_median"] - row["segment_regions"]["ms_median"], 3)
                print(json.dumps(row), flush=True)
                res["cases"].append(row)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
