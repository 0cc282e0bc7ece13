"""One rank of tests/test_hip_spread.py::test_two_rank_spread_on_one_gpu: torch.distributed over gloo, every rank on
cuda:0, P = 5 hypotheses (a ragged 3 + 2 split), infer_sequence(aggregate="mean", spread="cov") and (aggregate="reproj",
spread="std").
Usage (RANK, WORLD_SIZE, MASTER_ADDR, MASTER_PORT in the environment): python tests/spread_rank_worker.py OUT.pt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402


def main(out):
    import __graft_entry__ as ge
    from pafuse_amd.parallel import shard_range
    from tests.test_hip_pose_aggregate import infer
    dist.init_process_group("gloo", rank=int(os.environ["RANK"]), world_size=int(os.environ["WORLD_SIZE"]))
    try:
        ge.build()
        model, _ = ge.make_model(5, 2, depth=2)
        got = infer(model, aggregate="mean", spread="cov")
        reproj = infer(model, aggregate="reproj", spread="std")
        torch.save({"world": dist.get_world_size(), "local": list(shard_range(5, dist.get_rank(), dist.get_world_size())),
                    "pose": got["pose"], "cov": got["cov"], "std": got["std"], "reproj_std": reproj["std"]}, out)
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1])
