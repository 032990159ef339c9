"""One rank of a K-sharded iteration with the total-variation term on (launched by tests/test_gpu_tv.py as a fresh process, before any GPU
call, in the manner of tests/rank_worker.py: gloo on ONE GPU): one grad_only, then every rank writes tv() and the NLL to <out>_<rank>.npz.
usage: tv_rank_worker.py rank world port out"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, S, TV_WEIGHT = 4, 32, 0.02


def make_engine(rank, world):
    import torch
    from mfvi_dip_mia_amd.engine import ElboEngine
    from oracle import oracle as O
    eng = ElboEngine(S, S, task="den", K=K, input_depth=8, temp=1e-6, sigma=0.05, lr=1e-3, seed=7, rank=rank, world_size=world,
                     net_kwargs=dict(nd=(8, 16), nu=(8, 16), ns=(4, 4)), autotune=False, tv_weight=TV_WEIGHT)
    eng.set_target(torch.from_numpy(O.noisy(O.phantom(S, S, 7), 0.1, 7)))
    return eng


def main():
    rank, world, port, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port, RANK=str(rank), WORLD_SIZE=str(world))
    import numpy as np
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    eng = make_engine(rank, world)
    eng.grad_only(0, with_kl=False)
    torch.cuda.synchronize()
    np.savez("%s_%d.npz" % (out, rank), tv=eng.tv(), nll=eng.losses()[0], k_local=eng.K_local)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
