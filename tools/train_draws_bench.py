"""Host cost of a training step's random draws: train_draws = "torch" (one randint + one randn per clip, one bernoulli_ /
div_ / slice assignment per block, branch and part) against "device" (one q_sample launch that draws, one table launch per
part; noise stream v1), one JSON document.

    python tools/train_draws_bench.py [--out profiles/train_draws_bench.json] [--reps 7] [--steps 10] [--batch 37]
    rocprofv3 --kernel-trace --output-format csv -d DIR -o trace -- python tools/train_draws_bench.py --count-launches torch --out DIR/torch.json
    rocprofv3 --kernel-trace --output-format csv -d DIR -o trace -- python tools/train_draws_bench.py --count-launches device --out DIR/device.json
    python tools/train_draws_bench.py --merge-launch-counts torch=DIR_T/.../trace_kernel_trace.csv,device=DIR_D/.../trace_kernel_trace.csv

The default three-part model (depth 8, 'bf16x3') in train mode at B = 37, `model(inputs_2d, inputs_3d)` forward only and
forward + backward of the mpjpe loss.  Both legs run in one process, alternating inside every repeat; a measurement is `steps`
steps between two stream synchronisations, timed with the host's wall clock (the saving is host time) and with HIP events
alongside.  The 'torch' leg is the default path, which this mode leaves as it was: its repeats are the yardstick, their spread
the resolution.  Launch counts come from the profiler runs (runs of their own: tracing slows the host): --count-launches runs
ONE warm step of one leg between two marker launches, --merge-launch-counts counts the kernels between the markers.
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MARKER = "droppath_fill_kernel"        # the marker launch: a 4-row table filled through the unit entry (depth 1, B = 1, F = J = 1)


def count_between_markers(path):
    """launches of one traced step: the rows of a kernel trace between the first and the last marker-shaped launch"""
    with open(path, newline="") as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r.get("Start_Timestamp") or r.get("Start") or 0))
    names = [r.get("Kernel_Name") or r.get("Name") or "" for r in rows]
    grids = [int(r.get("Grid_Size") or r.get("Grid_Size_X") or 0) for r in rows]
    marks = [i for i, (n, g) in enumerate(zip(names, grids)) if MARKER in n and g <= 256]
    inside = names[marks[-2] + 1:marks[-1]]
    by = {}
    for n in inside:
        base = n.split("(")[0].split("<")[0]
        by[base] = by.get(base, 0) + 1
    draws = sum(v for k, v in by.items() if any(s in k for s in ("bernoulli", "random", "normal", "distribution", "Fill", "fill", "div",
                                                                   "copy", "Copy", "CatArray", "qsample", "droppath")))
    return {"launches": len(inside), "launches_of_draw_shaped_kernels": draws, "by_kernel": dict(sorted(by.items(), key=lambda kv: -kv[1]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_draws_bench.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=37)
    ap.add_argument("--count-launches", choices=("torch", "device"), default="")
    ap.add_argument("--merge-launch-counts", default="")
    a = ap.parse_args()
    if a.merge_launch_counts:
        doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
        doc["launches_of_one_forward_backward_step_under_rocprofv3"] = {
            leg: count_between_markers(path) for leg, path in (kv.split("=", 1) for kv in a.merge_launch_counts.split(","))}
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
        print(json.dumps({k: {x: y for x, y in v.items() if x != "by_kernel"}
                          for k, v in doc["launches_of_one_forward_backward_step_under_rocprofv3"].items()}))
        return

    import torch
    import __graft_entry__ as ge
    from pafuse_amd import _lib, ops
    from pafuse_amd import synthetic as gu
    ge.build()
    if not torch.cuda.is_available():
        raise SystemExit("train_draws_bench needs the GPU: a timing taken elsewhere says nothing")
    B = a.batch
    model, _ = ge.make_model(1, 1, seed=51, is_train=True)
    model.noise_seed = 1
    x2d = gu.synthetic_inputs_2d(B=B)[0].cuda()
    target = gu.synthetic_target_3d(B=B).cuda()

    def step(leg, backward):
        model.train_draws = leg
        if backward:
            model.zero_grad(set_to_none=True)
            pred = model(x2d, target)
            torch.mean(torch.norm(pred - target, dim=-1)).backward()
        else:
            with torch.no_grad():
                model(x2d, target)

    if a.count_launches:
        marker_model = __import__("pafuse_amd").MixSTE2(num_frame=1, num_joints=1, embed_dim_ratio=64, depth=1, drop_path_rate=0.5)
        _, keep, factor = marker_model.drop_path_tables("cuda")
        key = ops.train_key(0, 0, 0, 1, "cuda")
        step(a.count_launches, True), step(a.count_launches, True)     # warm
        torch.cuda.synchronize()
        ops.droppath_fill(key, 0, 1, 1, 1, 1, keep, factor)
        step(a.count_launches, True)
        ops.droppath_fill(key, 0, 1, 1, 1, 1, keep, factor)
        torch.cuda.synchronize()
        return

    def timed(leg, backward):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        for _ in range(a.steps):
            step(leg, backward)
        e1.record()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.steps, e0.elapsed_time(e1) / a.steps

    doc = {"what": f"D3DP train mode, three parts, depth 8, bf16x3, B = {B}: train_draws = 'device' against 'torch' (the default path), "
                   f"ms per step over {a.steps} steps between two synchronisations",
           "device": torch.cuda.get_device_name(0), "kernel_source_sha256": _lib.kernel_source_digest(), "reps": a.reps, "cases": []}
    for backward in (False, True):
        for leg in ("torch", "device"):
            timed(leg, backward)                                        # warm: code objects, streams, allocator
        wall, ev = {"torch": [], "device": []}, {"torch": [], "device": []}
        for _ in range(a.reps):
            for leg in ("torch", "device"):
                w, e = timed(leg, backward)
                wall[leg].append(w), ev[leg].append(e)

        def stats(v):
            return {"median": statistics.median(v), "min": min(v), "max": max(v), "spread_rel": (max(v) - min(v)) / statistics.median(v)}
        case = {"what": "forward + backward" if backward else "forward only", "B": B,
                "wall_ms_per_step": {k: stats(v) for k, v in wall.items()}, "event_ms_per_step": {k: stats(v) for k, v in ev.items()},
                "wall_ms": wall, "event_ms": ev,
                "device_minus_torch_wall_ms": statistics.median(wall["device"]) - statistics.median(wall["torch"]),
                "device_over_torch_wall": statistics.median(wall["device"]) / statistics.median(wall["torch"]),
                "clips_per_s_wall": {k: B / statistics.median(v) * 1e3 for k, v in wall.items()}}
        doc["cases"].append(case)
        print(json.dumps({k: v for k, v in case.items() if k not in ("wall_ms", "event_ms")}), flush=True)
    if os.path.exists(a.out):                                           # keep what earlier commands merged in
        old = json.load(open(a.out))
        doc.update({k: v for k, v in old.items() if k not in doc})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
