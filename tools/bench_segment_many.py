"""Grouped image sessions: what does ONE `segment_many` call over K sessions cost against the loop of K `segment` calls?

    python tools/bench_segment_many.py [--steps 20] [--warmup 3] [--layers 24] [--out profiles/segment_many_bench.json]

Tiny and full-width synthetic models, referring task, 640^2 images, K sessions x 3 sentences for K in {1, 2, 4, 8}, precision "f16x3", prefix caches
warm on both sides.  The loop of `segment` calls is existing code and is the yardstick; both run in the same process on the same sessions.
Each figure: wall time of a synchronous call (host work and read-back included), median of `--steps` calls after `--warmup`, plus the GPU time
between two events around the timed calls (tools/bench_session.py's `timed`).  No threshold is asserted.  One JSON with the commit hash and the
device's name is written to --out.
"""
import argparse
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_session import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--sessions", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--sentences", type=int, default=3)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--widths", nargs="+", default=["tiny", "full"])
    ap.add_argument("--commit", default=None, help="commit hash to record (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segment_many_bench.json"))
    args = ap.parse_args()
    from psalm_amd.config import PsalmConfig
    from psalm_amd.model import PSALM
    from psalm_amd.synthetic import fix_indices, make_state_dict, session_inputs
    commit = args.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    res = {"commit": commit, "device": torch.cuda.get_device_name(0), "precision": "f16x3", "task": "referring", "size": args.size,
           "sentences_per_session": args.sentences, "cases": []}
    for width in args.widths:
        cfg = PsalmConfig.tiny("referring") if width == "tiny" else PsalmConfig(num_layers=args.layers, seg_task="referring")
        sd = make_state_dict(cfg, seed=1)
        model = PSALM(cfg, sd, precision="f16x3", use_graphs=False)
        del sd
        reqs = []
        for k in range(max(args.sessions)):
            inp = fix_indices(session_inputs(cfg, "referring", args.sentences, size=args.size, seed=1 + k))
            kw = {k_: v for k_, v in inp.items() if k_ not in ("images", "labels", "is_thing_list")}
            reqs.append((model.encode_image(inp["images"][:1].cuda(), inp["seg_info"][0]), kw))
        for K in args.sessions:
            part = reqs[:K]
            model.segment_many(part)                             # (prefix caches warm on both sides)
            row = {"width": width, "layers": cfg.num_layers, "sessions": K, "prompts": K * args.sentences,
                   "prefix_rows": [s.prefix_len for s, _ in part]}
            row["segment_loop"] = timed(lambda: [model.segment(s, **kw) for s, kw in part], args.steps, args.warmup)
            row["segment_many"] = timed(lambda: model.segment_many(part), args.steps, args.warmup)
            row["ratio_loop_over_many"] = round(row["segment_loop"]["ms_median"] / row["segment_many"]["ms_median"], 3)
            print(json.dumps(row), flush=True)
            res["cases"].append(row)
        del model, reqs
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
