"""One rank of the data-parallel AUC check (TEST INFRASTRUCTURE; launched by tests/test_metrics_gpu.py through torch.distributed.run,
one process per GPU): every rank feeds ITS shard of one seeded evaluation set to metrics.AUC, then all ranks read the whole set's AUC
through the group.  Each rank checks the value against the numpy restatement on the whole set and that its own state is still its
shard's counts.  Prints 'DP_METRICS_OK <world> <auc>' on rank 0."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from ml_function_amd import metrics
    from tests import keras_auc_ref as ref
    rank, world, local = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)
    dist.barrier()
    per_rank = 50001
    rng = np.random.default_rng(2020)                               # the same evaluation set on every rank
    p = ref.skewed_scores(rng, per_rank * world)
    y = (rng.random(len(p)) < p).astype(np.float32)
    lo, hi = rank * per_rank, (rank + 1) * per_rank
    thr = ref.thresholds(200)
    m = metrics.AUC()
    for a in range(lo, hi, 4096):                                   # in batches, as an evaluation loop would
        b = min(a + 4096, hi)
        m.update_state(torch.tensor(y[a:b], device=device), torch.tensor(p[a:b], device=device))
    mine = np.stack(ref.counts(y[lo:hi], p[lo:hi], thr)).astype(np.float32)
    whole = ref.counts(y, p, thr)
    ok = True
    for _ in range(2):                                              # mid-epoch, repeatedly: the local state stays the shard's
        got = m.result_value(process_group=dist.group.WORLD)
        ok = ok and abs(got - float(ref.result(*whole, dt=np.float64))) <= 4 * 200 * 2.0 ** -24
        ok = ok and np.array_equal(m.confusion.cpu().numpy(), mine)
    every = [torch.zeros(1, device=device) for _ in range(world)]
    dist.all_gather(every, m.result(process_group=dist.group.WORLD).reshape(1))
    ok = ok and all(float(e) == float(every[0]) == got for e in every)
    flag = torch.tensor([1 if ok else 0], device=device)
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    ok = bool(int(flag))
    if rank == 0:
        print("DP_METRICS_%s %d %.6f" % ("OK" if ok else "FAILED", world, got), flush=True)
    dist.barrier()
    dist.destroy_process_group()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
