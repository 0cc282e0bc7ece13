"""Cost of the "device" noise source (fp64 Box-Muller inside finalize_seeded_kernel / noise_fill_kernel) against the loop
that reads a pre-drawn noise stack, one JSON document.

    python tools/noise_bench.py [--out profiles/device_noise_bench.json] [--reps 3] [--batches 1,64] [--no-graph]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o stats -- python tools/noise_bench.py --batches 1 --reps 1 --no-graph --out DIR/under_profiler.json
    python tools/noise_bench.py --merge-kernel-stats DIR/.../stats_kernel_stats.csv --out profiles/device_noise_bench.json

The loop at P = 20, T = 10, flip-TTA, 'bf16x3', eager and as a replayed graph.  Both legs are D3DP._sample_chunk calls, cut
along the clip axis exactly as ddim_sample cuts them, on operands made before the timed region: the 'torch' leg gets its
[n_draws,B,P,F,J,3] stack pre-drawn and pre-sliced (torch.randn's time is NOT credited to the new mode; the stack's copy
into the graph's static buffer is part of that leg, as it is in production), the 'device' leg gets its 16-byte keys.  The
'torch' leg runs the kernels and launches of the loop as it was before the noise source existed (finalize_kernel and
copy_kernel do what they did), so its repeats are the yardstick and their spread is the resolution.  HIP events around each
leg, warm, the legs alternating inside every repeat.  Kernel times come from the second command (a run of its own: tracing
slows the host) and are merged by the third.
"""
import argparse
import csv
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
P, T = 20, 10
KERNELS = ("finalize_kernel", "finalize_seeded_kernel", "noise_fill_kernel", "copy_kernel")


def merge_kernel_stats(path, out):
    rows = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Name") or r.get("KernelName") or ""
            m = re.search(r"([A-Za-z_]\w*)\(", name)          # "pafuse::finalize_kernel(pafuse::FinalizeParams)" -> finalize_kernel
            base = m.group(1) if m else ""
            if base in KERNELS:
                rows[base] = {k: r[k] for k in r if k != "Name"}
    doc = json.load(open(out)) if os.path.exists(out) else {}
    doc["kernel_stats_B1_under_rocprofv3"] = rows
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(rows, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_noise_bench.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batches", default="1,64")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--merge-kernel-stats", default="")
    a = ap.parse_args()
    if a.merge_kernel_stats:
        return merge_kernel_stats(a.merge_kernel_stats, a.out)

    import torch
    import __graft_entry__ as ge
    from pafuse_amd import _lib, ops
    from pafuse_amd import synthetic as gu
    ge.build()
    if not torch.cuda.is_available():
        raise SystemExit("noise_bench needs the GPU: a timing taken elsewhere says nothing")
    lib = _lib.load()
    model, _ = ge.make_model(P, T)
    steps = model.ddim_steps()
    n_draws = 1 + sum(1 for s in steps if not s.last)
    doc = {"what": "DDIM loop, P = 20, T = 10, flip-TTA, bf16x3: noise = 'device' against the loop on a pre-drawn noise stack",
           "device": torch.cuda.get_device_name(0), "kernel_source_sha256": _lib.kernel_source_digest(), "reps": a.reps, "cases": []}
    for B in [int(b) for b in a.batches.split(",")]:
        x2d, x2f = (t.cuda() for t in gu.synthetic_inputs_2d(B=B))
        bc = model.clips_per_launch(P, True)
        cuts = [(b0, min(B, b0 + bc)) for b0 in range(0, B, bc)]
        g = torch.Generator(device="cuda").manual_seed(1)
        stacks = [torch.randn(n_draws, b1 - b0, P, 27, 134, 3, device="cuda", generator=g) for b0, b1 in cuts]
        keys = [ops.noise_key(1, 0, b0, 0, "cuda") for b0, _ in cuts]

        def torch_leg():
            model.noise = "torch"
            return [model._sample_chunk(lib, x2d[b0:b1], x2f[b0:b1], z, steps, n_draws, True) for (b0, b1), z in zip(cuts, stacks)]

        def device_leg():
            model.noise = "device"
            return [model._sample_chunk(lib, x2d[b0:b1], x2f[b0:b1], None, steps, 0, True, key4=k, P=P) for (b0, b1), k in zip(cuts, keys)]

        def timed(leg):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = leg()
            e1.record()
            e1.synchronize()
            del out
            return e0.elapsed_time(e1)

        for graph in ([False] if a.no_graph else [False, True]):
            model.use_graph = graph
            model._graphs.clear()
            timed(torch_leg), timed(device_leg)                      # warm: code objects, weight images, captures
            ms = {"torch": [], "device": []}
            for _ in range(a.reps):
                ms["torch"].append(timed(torch_leg))
                ms["device"].append(timed(device_leg))
            t, d = statistics.median(ms["torch"]), statistics.median(ms["device"])
            case = {"B": B, "launches_per_call": len(cuts), "graph": graph, "ms": ms,
                    "median_ms": {"torch": t, "device": d},
                    "hypotheses_per_s": {"torch": B * P / t * 1e3, "device": B * P / d * 1e3},
                    "torch_spread_rel": (max(ms["torch"]) - min(ms["torch"])) / t,
                    "device_over_torch": d / t,
                    "noise_bytes_not_allocated": n_draws * B * P * 27 * 134 * 3 * 4}
            doc["cases"].append(case)
            print(json.dumps(case), flush=True)
        model.use_graph = False
        model._graphs.clear()
        del stacks
        torch.cuda.empty_cache()
    if os.path.exists(a.out):                                       # keep what earlier commands merged in
        old = json.load(open(a.out))
        doc.update({k: v for k, v in old.items() if k not in doc})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
