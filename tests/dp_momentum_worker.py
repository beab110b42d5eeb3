"""One rank of the data-parallel Keras SGD / RMSprop check (TEST INFRASTRUCTURE; launched by tests/test_optim_momentum_gpu.py through
torch.distributed.run, one process per GPU), tests/dp_rowwise_worker.py (whose model, batches and training loop it uses) with the
five variants of optim.SGD and optim.RMSprop: every rank trains ITS row shard of one batch through an XDeepFM with tableGrad="runs"
for 3 steps -- dense gradients through the bucketed all-reduce, the tables through the runs exchange (force_exchange, so a single rank
takes it too).  Then every rank's parameters and slots must be bit-identical (an all-gather of checksums), and rank 0 compares its
parameters with a full-batch run on its own GPU (the one-GPU path).  Prints 'DP_MOMENTUM_OK <world> <max rel err>' on rank 0."""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.dp_rowwise_worker import PER, batch, make_model, train  # noqa: E402


def checksum(model, opt):
    """Exact digest of every parameter and slot: their bits summed as int64 per tensor."""
    parts = []
    for p in model.parameters():
        st = opt.state.get(p, {})
        for t in (p.detach(),) + tuple(st[k] for k in ("rms", "momentum") if k in st):
            parts.append(t.contiguous().view(torch.int32).to(torch.int64).sum() * 1000003 + t.numel())
    return torch.stack(parts)


def main():
    import bench
    from ml_function_amd import optim
    rank, world, local = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    with bench.stdout_to_stderr():
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)
        dist.barrier()
    # rank 0's reference runs alone in its own group (every rank must create it): the dense gradients still go through a (no-op)
    # bucket, as the ranks' do, and the tables take the one-GPU path (a group of one rank, no force_exchange)
    solo = dist.new_group([0]) if world > 1 else dist.group.WORLD
    dense, idx, _ = batch(0, world)
    ok, err = True, 0.0
    makers = [("sgd", lambda ps, **kw: optim.SGD(ps, learning_rate=0.01, **kw)),
              ("sgd_momentum", lambda ps, **kw: optim.SGD(ps, learning_rate=0.01, momentum=0.9, **kw)),
              ("sgd_nesterov", lambda ps, **kw: optim.SGD(ps, learning_rate=0.01, momentum=0.9, nesterov=True, **kw)),
              ("rmsprop", lambda ps, **kw: optim.RMSprop(ps, learning_rate=0.001, **kw)),
              ("rmsprop_momentum", lambda ps, **kw: optim.RMSprop(ps, learning_rate=0.001, momentum=0.9, **kw))]
    for name, make_opt in makers:
        fi, model = make_model()
        model(dense[:PER], idx[:PER])
        opt = make_opt(model.parameters(), force_exchange=True)
        train(model, opt, slice(rank * PER, (rank + 1) * PER), world, dist.group.WORLD)
        torch.cuda.synchronize()
        assert all(p in opt._xbuf for p in (fi.sparse_embed.embeddings, fi.linear_embed.embeddings)), "the exchange path did not run"
        mine = checksum(model, opt)
        every = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(every, mine)
        same = all(torch.equal(e, every[0]) for e in every)
        ok = ok and same
        if rank == 0:
            fi_r, ref = make_model()
            ref(dense[:PER], idx[:PER])
            opt_r = make_opt(ref.parameters(), process_group=solo)      # world size 1 without force_exchange: the one-GPU path
            train(ref, opt_r, slice(0, PER * world), 1, solo)
            torch.cuda.synchronize()
            assert not opt_r._xbuf
            for (n, a), (_, b) in zip(model.named_parameters(), ref.named_parameters()):
                a, b = a.detach().double(), b.detach().double()
                if b.abs().max() > 0:
                    e = float((a - b).abs().max() / b.abs().max())
                    err = max(err, e)
                    ok = ok and e < 1e-4
                if world == 1 and not torch.equal(a, b):      # one shard: the exchange path is bit-for-bit the one-GPU path
                    print("differs bitwise: %s (%s)" % (n, name), flush=True)
                    ok = False
            print("%s: max rel err %.3e same=%s" % (name, err, same), flush=True)
    if rank == 0:
        print("DP_MOMENTUM_%s %d %.3e" % ("OK" if ok else "FAILED", world, err), flush=True)
    dist.barrier()
    dist.destroy_process_group()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
