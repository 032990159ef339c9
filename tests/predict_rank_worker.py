"""One rank of K-sharded posterior predictive sampling (launched by tests/test_gpu_predictive.py as a fresh process, before any GPU call):
ElboEngine(rank, world) with the gloo backend on ONE GPU, predict(N, target) — each rank draws its block of global sample indices, the
fp64 sums are all-reduced once, every rank finalizes — then rank 0 writes the maps and whether every rank holds the same ones.
usage: predict_rank_worker.py rank world port out.npz N"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KEYS = ("mean", "epi", "ale", "total", "err2", "mse_mc")


def make_engine(rank, world, pg=None):
    """The engine both the ranks and the single-rank comparison use (freshly initialised: mu / rho / BN follow the RNG spec, identical on
    every rank and in the single-rank process; a training step would differ in the last bits between the two gradient schedules)."""
    from mfvi_dip_mia_amd.engine import ElboEngine
    from oracle import oracle as O
    S = 64
    eng = ElboEngine(S, S, task="den", K=2, input_depth=8, temp=5.7e-7, sigma=1.5e-5, lr=1e-3, seed=9, rank=rank, world_size=world,
                     process_group=pg, net_kwargs=dict(nd=(8, 16, 16), nu=(8, 16, 16), ns=(4, 4, 4)), autotune=False)
    return eng, O.phantom(S, S, 9)


def main():
    rank, world, port, out, N = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], int(sys.argv[5])
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port, RANK=str(rank), WORLD_SIZE=str(world))
    import numpy as np
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    eng, gt = make_engine(rank, world)
    r = eng.predict(N, target=torch.from_numpy(gt))
    torch.cuda.synchronize()
    flat = torch.cat([r[k].reshape(-1) for k in KEYS])
    ref = flat.clone()
    dist.broadcast(ref, src=0)
    same = bool(torch.equal(ref, flat))
    flags = [None] * world
    dist.all_gather_object(flags, same)
    if rank == 0:
        np.savez(out, identical=np.array(flags), **{k: r[k].cpu().numpy() for k in KEYS})
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
