"""Image sessions: what does the mask decoder as ONE pass over all prompts of a call (PSALM.batch_decoder) save against the per-prompt loop?

    python tools/bench_decoder_batch.py [--steps 20] [--warmup 3] [--layers 24] [--out profiles/decoder_batch_bench.json]

Full-width synthetic model, precision "f16x3": the referring task at 640^2 and the region task at 1024^2, N prompts on one session for N in
{1, 2, 4, 8}, prefix cache warm.  Both settings run in ONE process on the same session and the same prompts, ALTERNATING call by call (off, on, off,
on, ...) after every shape was warmed up under both, so drift of the machine falls on both alike.  Each figure is over `--steps` (>= 20) synchronous
`segment(postprocess=False)` calls per setting: median and interquartile range of the wall time (host work included, one synchronisation behind the
call) and the median GPU time between two events around the call.  The two settings return the same words (tests/test_2[0-2]_batched_decoder_*), so
only time is compared.  One JSON with the commit hash and the device's name is written to --out.  Without a GPU the run fails and writes nothing.
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


def _stats(ms):
    q = statistics.quantiles(ms, n=4)
    return {"ms_median": round(statistics.median(ms), 4), "ms_iqr": round(q[2] - q[0], 4), "ms_min": round(min(ms), 4)}


def alternate(model, call, steps, warmup):
    """`call()` under batch_decoder off / on in turn: per setting the wall times (ms, synchronous) and the event times of `steps` calls"""
    wall, gpu = {False: [], True: []}, {False: [], True: []}
    for i in range(warmup + steps):
        for on in (False, True):
            model.batch_decoder = on
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if i >= warmup:
                wall[on].append((t1 - t0) * 1e3)
                gpu[on].append(e0.elapsed_time(e1))
    del model.batch_decoder
    return {("batched" if on else "loop"): dict(_stats(wall[on]), gpu_ms_median=round(statistics.median(gpu[on]), 4), calls=len(wall[on])) for on in (False, True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--prompts", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--cases", nargs="+", default=["referring:640", "region:1024"], help="task:image size")
    ap.add_argument("--commit", default=None, help="commit hash to record (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decoder_batch_bench.json"))
    args = ap.parse_args()
    if args.steps < 20:
        ap.error("--steps: at least 20 calls per setting")
    if not torch.cuda.is_available():
        sys.exit("bench_decoder_batch: no GPU visible (nothing written)")
    from psalm_amd.config import PsalmConfig
    from psalm_amd.model import PSALM
    from psalm_amd.synthetic import fix_indices, make_state_dict, session_inputs
    commit = args.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    res = {"commit": commit, "device": torch.cuda.get_device_name(0), "precision": "f16x3", "layers": args.layers, "steps": args.steps,
           "warmup": args.warmup, "decoder_batch_max": PSALM.decoder_batch_max, "order": "alternating: loop, batched, loop, batched, ...", "cases": []}
    for case in args.cases:
        task, size = case.split(":")
        size = int(size)
        cfg = PsalmConfig(num_layers=args.layers, seg_task=task)
        sd = make_state_dict(cfg, seed=1)
        model = PSALM(cfg, sd, precision="f16x3", use_graphs=False)
        del sd
        for N in args.prompts:
            inp = fix_indices(session_inputs(cfg, task, N, size=size, seed=1))
            kw = {k: v for k, v in inp.items() if k not in ("images", "labels", "is_thing_list")}
            sess = model.encode_image(inp["images"][:1].cuda(), inp["seg_info"][0])

            def call():
                torch.manual_seed(5)                              # (region task: the point sampler draws from the global generator)
                return model.segment(sess, postprocess=False, **kw)

            row = {"task": task, "size": size, "prompts": N, "mask_features": list(sess.mask_features_size), "levels": [list(s) for s in sess.shapes]}
            row.update(alternate(model, call, args.steps, args.warmup))
            row["loop_over_batched"] = round(row["loop"]["ms_median"] / row["batched"]["ms_median"], 3)
            row["gain_ms"] = round(row["loop"]["ms_median"] - row["batched"]["ms_median"], 4)
            print(json.dumps(row), flush=True)
            res["cases"].append(row)
            del sess
        del model
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
