"""Wall time of the D3DP flip-TTA sampler and of a training step at long clips (default 243 frames), one JSON line.

    python tools/long_clip_timing.py [--frames 243] [--P 20] [--T 1] [--dtype bf16x3] [--train-batch 4] [--reps 5]

Run it under `rocprofv3 --kernel-trace --stats -- python tools/long_clip_timing.py ...` to split the time by kernel: the
temporal attention is attn_long_kernel (forward) and attn_backward_long_kernel (backward) at frames > 144.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=243)
    ap.add_argument("--P", type=int, default=20)
    ap.add_argument("--T", type=int, default=1)
    ap.add_argument("--dtype", default="bf16x3")
    ap.add_argument("--train-batch", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    from pafuse_amd import synthetic as gu
    ge.build()
    dev = "cuda"
    F = a.frames
    out = {"frames": F, "P": a.P, "T": a.T, "dtype": a.dtype}

    model, _ = ge.make_model(a.P, a.T, device=dev, frames=F)
    model.precision = a.dtype
    x2d, x2f = gu.synthetic_inputs_2d(B=1, frames=F)
    x2d, x2f = x2d.to(dev), x2f.to(dev)
    with torch.no_grad():
        for _ in range(2):
            model(x2d, None, input_2d_flip=x2f)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            model(x2d, None, input_2d_flip=x2f)
        torch.cuda.synchronize()
    out["sample_ms"] = round((time.perf_counter() - t0) / a.reps * 1e3, 3)
    del model
    torch.cuda.empty_cache()

    B = a.train_batch
    model, _ = ge.make_model(1, 1, device=dev, is_train=True, frames=F)
    model.precision = a.dtype if a.dtype in ("f32", "bf16x3") else "bf16x3"
    x2d, _ = gu.synthetic_inputs_2d(B=B, frames=F)
    target = gu.synthetic_target_3d(B=B, frames=F).to(dev)
    x2d = x2d.to(dev)
    opt = torch.optim.AdamW(model.parameters(), lr=6e-5, weight_decay=0.1)
    torch.manual_seed(4321)

    def step():
        opt.zero_grad(set_to_none=True)
        loss = torch.mean(torch.norm(model(x2d, target) - target, dim=-1))
        loss.backward()
        opt.step()
        return loss

    for _ in range(2):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.reps):
        loss = step()
    torch.cuda.synchronize()
    out["train_B"] = B
    out["train_step_ms"] = round((time.perf_counter() - t0) / a.reps * 1e3, 3)
    out["train_loss_finite"] = bool(torch.isfinite(loss.detach()))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
