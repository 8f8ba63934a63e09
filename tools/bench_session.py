"""Image sessions: what does `encode_image` once + `segment` per prompt cost against `eval_seg` per (image, prompt) pair?

    python tools/bench_session.py [--steps 20] [--warmup 3] [--layers 24] [--out profiles/session_bench.json]

Full synthetic model, precision "f16x3".  For referring 640^2 and region 1024^2 and N in {1, 4, 8} prompts per image:
  (a) encode_image;  (b) one segment call with N prompts (prefix cache warm, as every call after the first is);  (b0) the first segment call
  of a session (prefix cache built);  (c) the one-shot way: eval_seg on a batch of N copies of the image, eager and through hipGraphs.
For N = 1 the derived break-even: the number of prompts per image from which encode_image + first segment + (k - 1) * segment beats k * eval_seg.
Each figure: wall time of a synchronous call (host work and the result read-back included, as bench.py's headline), median of `--steps`
calls after `--warmup`, plus the GPU time between two events around the timed calls.  One JSON with the commit hash is written to --out.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    wall = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t) * 1e3)
    e1.record()
    torch.cuda.synchronize()
    return {"ms_median": round(statistics.median(wall), 3), "ms_min": round(min(wall), 3), "ms_max": round(max(wall), 3),
            "ms_events_per_call": round(e0.elapsed_time(e1) / steps, 3), "steps": steps}


def break_even(encode, first, seg, one_shot):
    """smallest k with encode + first + (k - 1) * seg < k * one_shot (k prompts on one image, one per call); None if segment is not the cheaper call"""
    if seg >= one_shot:
        return None
    return max(1, int((encode + first - seg) / (one_shot - seg)) + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--prompts", type=int, nargs="+", default=[1, 4, 8])
    ap.add_argument("--cases", nargs="+", default=["referring:640", "region:1024"])
    ap.add_argument("--commit", default=None, help="commit hash to record (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "session_bench.json"))
    args = ap.parse_args()
    from psalm_amd.config import PsalmConfig
    from psalm_amd.model import PSALM
    from psalm_amd.synthetic import fix_indices, make_state_dict, session_inputs
    commit = args.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    res = {"commit": commit, "device": torch.cuda.get_device_name(0), "precision": "f16x3", "layers": args.layers, "cases": []}
    for case in args.cases:
        task, size = case.split(":")
        size = int(size)
        cfg = PsalmConfig(num_layers=args.layers, seg_task=task)
        sd = make_state_dict(cfg, seed=1)
        eager = PSALM(cfg, sd, precision="f16x3", use_graphs=False)         # (one model: `use_graphs` is switched on for the graph leg only)
        del sd
        for n in args.prompts:
            inp = fix_indices(session_inputs(cfg, task, n, size=size, seed=1))
            inp["images"] = inp["images"].cuda()
            kw = {k: v for k, v in inp.items() if k not in ("images", "labels")}
            img, info = inp["images"][:1], inp["seg_info"][0]
            row = {"task": task, "size": size, "prompts": n}
            row["encode_image"] = timed(lambda: eager.encode_image(img, info), args.steps, args.warmup)
            sess = eager.encode_image(img, info)
            eager.segment(sess, **kw)
            row["prefix_rows"] = sess.prefix_len
            row["session_bytes"] = sess.nbytes()
            row["segment"] = timed(lambda: eager.segment(sess, **kw), args.steps, args.warmup)

            def first():
                sess.prefix_key = None                       # forget the prefix: the next call rebuilds the cache
                eager.segment(sess, **kw)
            row["segment_first_call"] = timed(first, args.steps, args.warmup)
            row["eval_seg_eager"] = timed(lambda: eager.eval_seg(**inp), args.steps, args.warmup)
            eager.use_graphs = True
            try:
                row["eval_seg_graphs"] = timed(lambda: eager.eval_seg(**inp), args.steps, max(args.warmup, 3))
            finally:
                eager.use_graphs = False
                eager._graphs.clear()
            a, b = row["encode_image"]["ms_median"], row["segment"]["ms_median"]
            row["eval_seg_per_prompt_ms"] = {k: round(row[k]["ms_median"] / n, 3) for k in ("eval_seg_eager", "eval_seg_graphs")}
            row["segment_per_prompt_ms"] = round(b / n, 3)
            if n == 1:                                       # prompts asked one at a time: from how many per image is the session ahead?
                row["break_even_prompts"] = {k: break_even(a, row["segment_first_call"]["ms_median"], b, row[k]["ms_median"])
                                             for k in ("eval_seg_eager", "eval_seg_graphs")}
            print(json.dumps(row), flush=True)
            res["cases"].append(row)
        del eager
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
