"""Train one of the re-hosted CTR models on synthetic Criteo-shaped data: the counterpart of the reference's
example/ctr_example/un_seq.py (Adam + binary cross-entropy + AUC, :55-66), on the HIP layers.

  python examples/train_ctr.py --model XDeepFM --steps 200
  python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 examples/train_ctr.py --model XDeepFM

The input side is the reference's too: the raw click log is a CSV-shaped pandas frame (string categories with missing values, dense
columns with NaNs) that goes through the field-index front end ml_function_amd.data_prepare (sparse_fea_deal: fillna('-1') ->
astype(str) -> label encoding, one sparseFea per column; dense_fea_deal: fillna(mode) -> min-max scaling; kon/utils/data_prepare.py:
85-100, 294-301); then (:335-337) the encoded table is sliced, shuffled with a
2048-element buffer, repeated, batched and prefetched by ml_function_amd.data.data_pipeline (host -> device copies on a
side stream); the loss is Keras' compiled loss: binary cross-entropy + the layers' regularisation terms (the l2(emb_reg)
of every embedding table, interactive_layer.py:217); the optimiser is Keras' 'adam' (lr 1e-3, epsilon 1e-7).
Data parallel: every rank trains on its own shard of the table, dense gradients go through one bucketed all-reduce
(ml_function_amd.dp.allreduce_module_grads), the embedding tables exchange only the rows their shards touched
(dp.exchange_sparse_rows) -- or, with --optimizer keras* --dp-tables runs, their compacted gradient runs (the runs exchange of
optim.Adam / Adagrad / Ftrl).  Labels come from a fixed random "teacher" so that the AUC has something to learn.
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pandas as pd  # noqa: E402

from ml_function_amd import data, dp, losses, metrics, models, optim, schedules  # noqa: E402
from ml_function_amd.data_prepare import data_prepare  # noqa: E402
from ml_function_amd.layers.base import collect_regularization_loss  # noqa: E402


def make_raw_log(rng, vocab, n_dense, rows, teacher):
    """A synthetic click log as it would come out of a CSV: (sparse frame of STRING categories with ~2 % missing values, dense frame
    of floats with ~2 % NaNs, label [rows]).  The labels follow a fixed random teacher on the raw values."""
    idx = np.stack([np.minimum(rng.zipf(1.3, rows) - 1, v - 1) for v in vocab], 1)
    dense = rng.random((rows, n_dense)) * 100.0
    logit = sum(teacher[f][idx[:, f]] for f in range(len(vocab))) + (dense / 100.0) @ teacher["dense"]
    y = (rng.random(rows) < 1.0 / (1.0 + np.exp(-logit))).astype(np.float32)
    sparse = pd.DataFrame({"C%d" % (f + 1): np.where(rng.random(rows) < 0.02, None, np.char.add("v", idx[:, f].astype("U"))) for f in range(len(vocab))})
    dense_df = pd.DataFrame({"I%d" % (i + 1): np.where(rng.random(rows) < 0.02, np.nan, dense[:, i]) for i in range(n_dense)})
    return sparse, dense_df, y


def make_schedule(args):
    """--lr-schedule and its parameters as a schedules.* object (Keras' tf.keras.optimizers.schedules), or the float --lr."""
    if args.lr_schedule == "none":
        return args.lr
    if args.lr_schedule == "exponential":
        return schedules.ExponentialDecay(args.lr, args.lr_decay_steps, args.lr_decay_rate, staircase=args.lr_staircase)
    if args.lr_schedule == "inverse-time":
        return schedules.InverseTimeDecay(args.lr, args.lr_decay_steps, args.lr_decay_rate, staircase=args.lr_staircase)
    if args.lr_schedule == "polynomial":
        return schedules.PolynomialDecay(args.lr, args.lr_decay_steps, end_learning_rate=args.lr_end, power=args.lr_power,
                                         cycle=args.lr_cycle)
    bounds = [int(x) for x in args.lr_boundaries.split(",") if x]
    values = [float(x) for x in args.lr_values.split(",") if x]
    return schedules.PiecewiseConstantDecay(bounds, values)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="XDeepFM", choices=["FM", "DeepFM", "DCN", "XDeepFM", "AutoInt", "NFM", "AFM"])
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--batch", type=int, default=4096, help="per-GPU batch")
    ap.add_argument("--fields", type=int, default=26)
    ap.add_argument("--dense", type=int, default=13)
    ap.add_argument("--embed-dim", type=int, default=16)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--cin-precision", default="f32", choices=["f32", "bf16"],
                    help="XDeepFM only: bf16 = the CIN's labelled bf16 training mode (one bf16 MFMA per product in its three GEMM "
                         "launches, ~1e-3 relative error); f32 = the exact chain")
    ap.add_argument("--optimizer", default="torch", choices=["torch", "keras", "keras-lazy", "keras-adagrad", "keras-ftrl", "keras-sgd", "keras-rmsprop",
                                                                     "keras-adadelta", "keras-adamax", "keras-nadam"],
                    help="torch = torch.optim.Adam on dense table gradients; keras = ml_function_amd.optim.Adam (Keras' epsilon placement), "
                         "on one GPU with the tables updated in place from the batch's gradient runs (tableGrad='runs'); keras-lazy = the "
                         "same with LazyAdam tables (only touched rows change: a labelled deviation from the reference); keras-adagrad / "
                         "keras-ftrl = ml_function_amd.optim.Adagrad / Ftrl (Keras' defaults and semantics, the tables in place as for "
                         "keras; Ftrl's strengths: --ftrl-*); keras-sgd / keras-rmsprop = ml_function_amd.optim.SGD / RMSprop (--momentum, "
                         "--nesterov, --rho; RMSprop without momentum is what Keras' optimizer='rmsprop' builds); keras-adadelta / keras-adamax = "
                         "ml_function_amd.optim.Adadelta / Adamax (--rho; --beta-1, --beta-2); keras-nadam = ml_function_amd.optim.Nadam (--beta-1, "
                         "--beta-2, --schedule-decay; like Keras' it takes no schedule and no decay).  Data parallel: the tables keep their dense gradients and the sparse row "
                         "exchange unless --dp-tables runs")
    ap.add_argument("--dp-tables", default="dense", choices=["dense", "runs"],
                    help="data parallel with --optimizer keras*: runs = the tables take tableGrad='runs' and the optimizer's runs "
                         "exchange (each rank's compacted gradient runs all-gathered, one merged update per replica, no [V,K] gradient, "
                         "no host sync after the first step); dense = the dense table gradients and dp.exchange_sparse_rows.  The default "
                         "stays dense: the runs exchange's all-gather at N > 1 ranks has not been timed on hardware yet (one GPU only)")
    ap.add_argument("--sweep-period", type=int, default=None, metavar="N",
                    help="with --optimizer keras: deferred Keras mode (optim.Adam(sweep_period=N)) -- the untouched table rows catch up "
                         "on read and in one rolling slice of 1/N of the table per step instead of a whole-table sweep per step; the "
                         "same bits as keras after a flush (state_dict).  8 is a good choice (DESIGN 6e); default: the per-step sweep")
    ap.add_argument("--amsgrad", action="store_true",
                    help="with --optimizer keras: Keras' Adam(amsgrad=True) (optim.Adam(amsgrad=True): a third slot vhat, the running "
                         "maximum of v, in the denominator); not with --sweep-period")
    ap.add_argument("--ftrl-lr-power", type=float, default=-0.5, help="--optimizer keras-ftrl: learning_rate_power (<= 0)")
    ap.add_argument("--ftrl-l1", type=float, default=0.0, help="--optimizer keras-ftrl: l1_regularization_strength")
    ap.add_argument("--ftrl-l2", type=float, default=0.0, help="--optimizer keras-ftrl: l2_regularization_strength")
    ap.add_argument("--ftrl-l2-shrinkage", type=float, default=0.0, help="--optimizer keras-ftrl: l2_shrinkage_regularization_strength")
    ap.add_argument("--momentum", type=float, default=0.0, help="--optimizer keras-sgd / keras-rmsprop: momentum, in [0, 1]")
    ap.add_argument("--nesterov", action="store_true", help="--optimizer keras-sgd: Nesterov momentum")
    ap.add_argument("--rho", type=float, default=None, help="--optimizer keras-rmsprop / keras-adadelta: rho (Keras' defaults: 0.9 / 0.95)")
    ap.add_argument("--beta-1", type=float, default=0.9, help="--optimizer keras-adamax / keras-nadam: beta_1")
    ap.add_argument("--beta-2", type=float, default=0.999, help="--optimizer keras-adamax / keras-nadam: beta_2")
    ap.add_argument("--schedule-decay", type=float, default=0.004, help="--optimizer keras-nadam: schedule_decay")
    ap.add_argument("--lr-schedule", default="none", choices=["none", "exponential", "inverse-time", "polynomial", "piecewise"],
                    help="with --optimizer keras*: a Keras learning-rate schedule (ml_function_amd.schedules) starting at --lr, evaluated "
                         "on the GPU from the optimizer's step counter -- it stays inside the captured graph.  exponential / inverse-time: "
                         "--lr-decay-steps, --lr-decay-rate, --lr-staircase; polynomial: --lr-decay-steps, --lr-end, --lr-power, --lr-cycle; "
                         "piecewise: --lr-boundaries, --lr-values (--lr is not used)")
    ap.add_argument("--lr-decay-steps", type=int, default=1000)
    ap.add_argument("--lr-decay-rate", type=float, default=0.96)
    ap.add_argument("--lr-staircase", action="store_true")
    ap.add_argument("--lr-end", type=float, default=1e-4, help="polynomial: end_learning_rate")
    ap.add_argument("--lr-power", type=float, default=1.0, help="polynomial: power")
    ap.add_argument("--lr-cycle", action="store_true", help="polynomial: cycle")
    ap.add_argument("--lr-boundaries", default="", help="piecewise: comma-separated step boundaries (at most 32), e.g. 100,200")
    ap.add_argument("--lr-values", default="", help="piecewise: one rate more than boundaries, e.g. 1e-3,5e-4,1e-4")
    ap.add_argument("--lr-decay", type=float, default=0.0,
                    help="with --optimizer keras*: Keras' legacy decay= keyword, lr / (1 + decay * iterations), applied after the "
                         "schedule; also computed on the GPU")
    ap.add_argument("--keras-auc", action="store_true",
                    help="also keep the reference's compiled metric, tf.keras.metrics.AUC() (metrics.AUC: 200 thresholds, stateful), "
                         "updated inside the training step -- so inside the captured graph -- over every batch; the log line then "
                         "prints the running Keras AUC beside the logged batch's exact one (data parallel: the whole group's)")
    ap.add_argument("--keras-metrics", action="store_true",
                    help="also keep what Keras reports for a compiled model at every batch: the running loss (metrics.Mean over the "
                         "batch loss, the progress bar's `loss`), metrics.BinaryCrossentropy (the LogLoss of the CTR papers) and "
                         "metrics.BinaryAccuracy, updated inside the training step -- so inside the captured graph -- and read at the "
                         "logging steps without a launch (data parallel: the whole group's)")
    ap.add_argument("--no-graph", action="store_true",
                    help="run every step eagerly (default on one GPU: the whole step -- forward, backward, Adam -- is captured once "
                         "into a HIP graph and replayed; the C ABI neither allocates nor synchronises, so it is capture-safe)")
    args = ap.parse_args()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    if world > 1:
        dist.init_process_group("nccl", device_id=device)
    rng0 = np.random.default_rng(2020)
    vocab = [int(v) for v in np.exp(rng0.uniform(np.log(10), np.log(2e5), args.fields))]
    teacher = {f: rng0.normal(0, 0.5, v).astype(np.float32) for f, v in enumerate(vocab)}
    teacher["dense"] = rng0.normal(0, 0.5, args.dense).astype(np.float32)
    # raw log -> field-index front end -> ids + descriptors.  LabelEncoder ids are ranks in the sorted set of the values PRESENT, so
    # the encoder must see the same log on every rank or one raw category would land in different embedding rows on different
    # replicas (and the averaged gradients would mix unrelated categories): the WHOLE log is drawn from one common seed and encoded
    # identically everywhere; a rank then keeps its own row shard of the encoded frame.
    per_rank = args.steps * args.batch // 2                                                  # repeat(2) makes `steps` batches
    raw_sparse, raw_dense, labels = make_raw_log(np.random.default_rng(1000), vocab, args.dense, per_rank * world, teacher)
    prep = data_prepare(batch_size=args.batch)
    ids_df, info = prep.sparse_fea_deal(raw_sparse, embed_dim=args.embed_dim)
    dense_df, _ = prep.dense_fea_deal(raw_dense)
    lo, hi = rank * per_rank, (rank + 1) * per_rank
    ids_df, dense_df, labels = ids_df.iloc[lo:hi], dense_df.iloc[lo:hi], labels[lo:hi]
    single = args.model == "XDeepFM"
    keras = args.optimizer != "torch"
    if not keras and (args.lr_schedule != "none" or args.lr_decay != 0.0):
        ap.error("--lr-schedule / --lr-decay need --optimizer keras* (torch.optim.Adam's rate is a host value baked into the captured "
                 "graph; the Keras optimizers of ml_function_amd.optim compute theirs on the GPU)")
    lr = make_schedule(args)
    if args.sweep_period is not None and args.optimizer != "keras":
        ap.error("--sweep-period needs --optimizer keras")
    if args.amsgrad and (args.optimizer != "keras" or args.sweep_period is not None):
        ap.error("--amsgrad needs --optimizer keras and no --sweep-period")
    if args.sweep_period is not None and world > 1 and args.dp_tables != "runs":
        ap.error("--sweep-period needs --dp-tables runs when data parallel (dense table gradients are not deferred)")
    fi = models.FeatureInput(sparseInfo=info, useLinear=args.model != "DCN" and args.model != "AutoInt", useAddLinear=single,
                             useFlattenLinear=True, tableGrad="runs" if keras and (world == 1 or args.dp_tables == "runs") else "dense")
    body = {"FM": models.FM, "DeepFM": models.DeepFM, "DCN": models.DCN, "AutoInt": models.AutoInt, "NFM": models.NFM,
            "AFM": models.AFM, "XDeepFM": lambda: models.XDeepFM(conv_size=[128, 128, 128], precision=args.cin_precision)}[args.model]()
    torch.manual_seed(0)  # identical replicas
    model = models.CTRModel(fi, body).to(device)
    table = (dense_df.to_numpy(np.float32), ids_df.to_numpy(np.int64), labels)
    use_dense = args.model not in ("FM", "AutoInt", "AFM")
    model(torch.tensor(table[0][:args.batch], device=device) if use_dense else None,
          torch.tensor(table[1][:args.batch], device=device))  # builds the lazily created weights
    tables = [p for n, p in model.named_parameters() if n.endswith("embeddings")]
    # l2(emb_reg) of the tables: added analytically after the sparse exchange (see dp.add_table_l2_grad_), identically per replica
    table_l2 = {id(m.embeddings): m.table_l2_ranges() for m in model.modules() if hasattr(m, "table_l2_ranges") and m.built}
    others = [p for n, p in model.named_parameters() if not n.endswith("embeddings")]
    use_graph = world == 1 and not args.no_graph
    if args.optimizer == "keras-adagrad":       # Keras' Adagrad; tables in "runs" mode get their l2 inside the update
        opt = optim.Adagrad(model.parameters(), learning_rate=lr, decay=args.lr_decay)
    elif args.optimizer == "keras-sgd":         # Keras' SGD (plain, momentum, Nesterov), likewise
        opt = optim.SGD(model.parameters(), learning_rate=lr, momentum=args.momentum, nesterov=args.nesterov, decay=args.lr_decay)
    elif args.optimizer == "keras-rmsprop":     # Keras' RMSprop; without momentum every row's rms decays at every step (one sweep)
        opt = optim.RMSprop(model.parameters(), learning_rate=lr, rho=0.9 if args.rho is None else args.rho, momentum=args.momentum,
                            epsilon=1e-7,
                            decay=args.lr_decay)
    elif args.optimizer == "keras-adadelta":    # Keras' Adadelta, likewise (row-local: only regularised fields are swept)
        opt = optim.Adadelta(model.parameters(), learning_rate=lr, rho=0.95 if args.rho is None else args.rho, epsilon=1e-7,
                             decay=args.lr_decay)
    elif args.optimizer == "keras-adamax":      # Keras' Adamax, likewise; its step size is formed on the GPU from the step counter
        opt = optim.Adamax(model.parameters(), learning_rate=lr, beta_1=args.beta_1, beta_2=args.beta_2, epsilon=1e-7,
                           decay=args.lr_decay)
    elif args.optimizer == "keras-nadam":       # Keras' Nadam: m and v of every row decay at every step (one sweep), a number as rate
        if args.lr_schedule != "none" or args.lr_decay != 0.0:
            ap.error("--optimizer keras-nadam takes neither --lr-schedule nor --lr-decay (Keras' Nadam refuses both)")
        opt = optim.Nadam(model.parameters(), learning_rate=lr, beta_1=args.beta_1, beta_2=args.beta_2, epsilon=1e-7,
                          schedule_decay=args.schedule_decay)
    elif args.optimizer == "keras-ftrl":        # Keras' Ftrl, likewise
        opt = optim.Ftrl(model.parameters(), learning_rate=lr, learning_rate_power=args.ftrl_lr_power,
                         l1_regularization_strength=args.ftrl_l1, l2_regularization_strength=args.ftrl_l2,
                         l2_shrinkage_regularization_strength=args.ftrl_l2_shrinkage, decay=args.lr_decay)
    elif keras:     # Keras 'adam' (un_seq.py:61) with Keras' numerics; tables in "runs" mode get their l2 inside the update
        opt = optim.Adam(model.parameters(), learning_rate=lr, epsilon=1e-7, lazy_tables=args.optimizer == "keras-lazy",
                         sweep_period=args.sweep_period, decay=args.lr_decay, amsgrad=args.amsgrad)
    else:
        opt = torch.optim.Adam(model.parameters(), lr=args.lr, eps=1e-7, capturable=use_graph)      # Keras 'adam' (un_seq.py:61)
    keras_auc = metrics.AUC().build(device) if args.keras_auc else None      # the state exists before any capture
    # (the same for Keras' running loss, LogLoss and accuracy)
    keras_metrics = ([metrics.Mean(name="loss").build(device), metrics.BinaryCrossentropy().build(device),
                      metrics.BinaryAccuracy().build(device)] if args.keras_metrics else None)
    pipe = data.data_pipeline(table, batch_size=args.batch, shuffle_buffer=2048, repeat=2, prefetch=2, seed=rank, device=device)

    def train_step(dense, idx, y):
        """forward + loss + backward + (data-parallel exchange) + Adam; returns (bce, p) of the batch"""
        opt.zero_grad(set_to_none=True)
        out = model(dense if use_dense else None, idx)
        p = out[:, 1] if out.shape[1] == 2 else out[:, 0]
        bce = losses.binary_crossentropy(p, y, eps=1e-6)       # clip + BCE + mean: one launch (ml_function_amd/losses.py)
        loss = (bce + collect_regularization_loss(model, skip_tables=True)) / world
        loss.backward()
        if world > 1:
            bucket = dp.GradBucket.for_params(others)
            bucket.copy_from_grads(others)
            bucket.all_reduce()
            bucket.assign_to_grads(others)
            offs = fi.sparse_embed.offsets
            rows = (idx + offs).reshape(-1)
            for t in tables:
                if t.grad is not None:          # (runs tables have no .grad: the optimizer exchanges their runs and adds their l2 itself)
                    dp.exchange_sparse_rows(t.grad, rows)
        for t in tables:
            if t.grad is not None and table_l2.get(id(t)):
                dp.add_table_l2_grad_(t.grad, t.detach(), table_l2[id(t)])
        opt.step()
        if keras_auc is not None:
            keras_auc.update_state(y, p)            # one launch, no host synchronisation
        if keras_metrics is not None:               # one launch each, likewise; the launch also leaves the result
            pc = p.detach().contiguous()            # (a column of the softmax head is a strided view: one copy for both readers)
            keras_metrics[0].update_state(bce)
            keras_metrics[1].update_state(y, pc)
            keras_metrics[2].update_state(y, pc)
        return bce.detach(), p.detach()

    graph, static = None, None
    for step, (dense, idx, y) in enumerate(pipe):
        full = idx.shape[0] == args.batch            # (the last batch of the pipeline can be short: it runs eagerly)
        if use_graph and full:
            if graph is None:
                # static input buffers; three eager steps on a side stream (lazy initialisations, allocator warm-up), then capture
                static = [torch.empty_like(dense), torch.empty_like(idx), torch.empty_like(y)]
                for dst, src in zip(static, (dense, idx, y)):
                    dst.copy_(src)
                # (the warm-up steps are real optimizer steps: model and Adam state are put back afterwards, so the captured run follows
                # the eager one step for step)
                saved_model = {k: v.clone() for k, v in model.state_dict().items()}
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    for _ in range(3):
                        train_step(*static)
                torch.cuda.current_stream().wait_stream(side)
                model.load_state_dict(saved_model)
                if keras:
                    opt.reset_()                    # slots, row stamps and the device step counter, in place
                else:
                    for st_ in opt.state.values():      # Adam's moments and step count back to "never stepped" (in place: the capture keeps these tensors)
                        for v in st_.values():
                            if torch.is_tensor(v):
                                v.zero_()
                if keras_auc is not None:
                    keras_auc.reset_states()        # the warm-up batches do not count (in place: the capture keeps the state)
                for m in keras_metrics or ():
                    m.reset_states()
                graph = torch.cuda.CUDAGraph()
                opt.zero_grad(set_to_none=True)
                with torch.cuda.graph(graph):
                    static_out = train_step(*static)
            for dst, src in zip(static, (dense, idx, y)):
                dst.copy_(src)
            graph.replay()
            bce, p = static_out
        else:
            bce, p = train_step(dense, idx, y)
        if step % 20 == 0 or step == len(pipe) - 1:
            # (every rank takes part in the group read; result_value() is also where scores outside [0, 1] would raise)
            running = "" if keras_auc is None else "  keras auc (running) %.4f" % keras_auc.result_value(
                process_group=dist.group.WORLD if world > 1 else None)
            if keras_metrics is not None:
                group = dist.group.WORLD if world > 1 else None
                running += "  keras " + "  ".join("%s %.4f" % (m.name, float(m.result(process_group=group))) for m in keras_metrics)
            # (the rate of the NEXT step: the counter has advanced; computed on the device, read here)
            rate = float(opt.current_learning_rate()) if keras else args.lr
            if rank == 0:
                print("step %4d  loss %.4f  auc %.4f  lr %.3e%s" % (step, float(bce), metrics.auc(y, p), rate, running), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
