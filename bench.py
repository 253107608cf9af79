#!/usr/bin/env python3
"""Flagship benchmark: FedSTIL ResNet-50 federated round throughput on MI355X.

Measures the BASELINE.json metric — images/sec (whole node) per federated
round, FedSTIL ResNet-50, one simulated edge client per GPU, bf16 compute,
synthetic data, random-init weights.  One bench step == one communication
round: prototype-capture forward over the task loader (frozen backbone) +
head training epoch on prototype features + upload / aggregate / dispatch
(RCCL collectives when N > 1).

Launch (the driver's contract):
  python bench.py --gpus 1 --steps K --warmup W
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
      --master-addr 127.0.0.1 bench.py --gpus N --steps K --warmup W

A plain run does only what the headline figure needs: set up, W warm-up
rounds, K timed rounds, one JSON result line.  Two options add to that:
  --dump-outputs DIR   after the timed rounds, write what the last timed
                       round produced (the uploads the server received and
                       the round's training loss / accuracy) as
                       DIR/<name>.npy, so two builds can be compared output
                       for output on identical seeded inputs
  --full               also measure Rank-1 on the synthetic tasks (the
                       BASELINE metric pairs throughput with Rank-1) and
                       report it as "rank1" in the result line

Weak scaling: per-GPU work is fixed (one client per rank, same task size);
the whole-job value aggregates over all ranks.
"""

import argparse
import json
import os
import sys
import time

REPO_ROOT = os.path.dirname(os.path.abspath(__file__))
if REPO_ROOT not in sys.path:
    sys.path.insert(0, REPO_ROOT)

# benchmark mode: no ckpt audit trail in the timed loop; MIOpen auto-tuned
# conv algos (see tools/utils.same_seeds)
os.environ.setdefault("FLREID_DISABLE_CKPT", "1")
os.environ.setdefault("FLREID_FAST_CONV", "1")
os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
os.environ.setdefault("FLREID_GPU_AUGMENT", "1")
# bf16 wire for the upload gather: halves xGMI traffic (the FedSTIL upload is
# ~125 MB/client in fp32); the aggregation itself stays fp32 on-device
os.environ.setdefault("FLREID_COMM_DTYPE", "bf16")
# FAST-mode find lands fresh shapes on the 1.5-15 ms naive reference convs
# (profiled at 62% of a steady round before the fixed-shape eval tails);
# with the naive solvers off it picks a real CK/igemm kernel instead
os.environ.setdefault("MIOPEN_DEBUG_CONV_DIRECT_NAIVE_CONV_FWD", "0")
os.environ.setdefault("MIOPEN_DEBUG_CONV_DIRECT_NAIVE_CONV_BWD", "0")
os.environ.setdefault("MIOPEN_DEBUG_CONV_DIRECT_NAIVE_CONV_WRW", "0")


def _seed_miopen_db():
    """Seed MIOPEN_USER_DB_PATH from the shipped pre-tuned find DB
    (flreid_amd/data/miopen_udb/) so every box starts from the same conv-algo
    picks — FIND_MODE=FAST occasionally landed on im2col/naive fallbacks for
    the eval-path shapes, a 10 %+ box lottery.  MIOpen writes to the user DB
    path, so the files are copied somewhere writable first."""
    if "MIOPEN_USER_DB_PATH" in os.environ:
        return
    src = os.path.join(REPO_ROOT, "flreid_amd", "data", "miopen_udb")
    if not os.path.isdir(src):
        return
    import shutil
    import tempfile
    # per-rank dir: MIOpen WRITES to the user DB path, and the driver's
    # 8-rank SCALE launch would otherwise race all ranks on one file set
    rank = os.environ.get("RANK", "0")
    # per-user too: another account's copy in a shared temp dir is read-only
    # to this one
    dst = os.path.join(tempfile.gettempdir(),
                       f"flreid_miopen_udb_u{os.getuid()}_r{rank}")
    os.makedirs(dst, exist_ok=True)
    for f in os.listdir(src):
        if not f.endswith(".txt"):
            continue
        t = os.path.join(dst, f)
        if not os.path.exists(t):
            shutil.copy(os.path.join(src, f), t)
    os.environ["MIOPEN_USER_DB_PATH"] = dst


_seed_miopen_db()

import torch  # noqa: E402


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=8)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--model", type=str, default="resnet50")
    p.add_argument("--method", type=str, default="fedstil")
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--img", type=str, default="128x64")
    p.add_argument("--ids", type=int, default=64,
                   help="identities per synthetic task")
    p.add_argument("--imgs-per-id", type=int, default=8,
                   help="train images per identity per task")
    p.add_argument("--num-classes", type=int, default=8000)
    p.add_argument("--lambda-k", type=int, default=2000,
                   help="FedSTIL exemplar budget.  The reference's ResNet-50 "
                        "config uses 12000 over the thousands of identities "
                        "of 5 real datasets (a few exemplars per id); scaled "
                        "to this synthetic 64-id task it gives m=32 per id — "
                        "a proportionally LARGER per-id rehearsal load")
    p.add_argument("--lambda-l1", type=float, default=1e-4)
    p.add_argument("--cpu", action="store_true", help="debug on CPU")
    p.add_argument("--channels-last", dest="channels_last",
                   action="store_true", default=True,
                   help="NHWC weights (MIOpen channels-last conv path; default)")
    p.add_argument("--no-channels-last", dest="channels_last",
                   action="store_false")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="write the last timed round's outputs to DIR/*.npy")
    p.add_argument("--full", action="store_true",
                   help="also run the post-benchmark Rank-1 validation and "
                        "report it in the result line")
    return p.parse_args()


# --dump-outputs budget: 48 MB of float32 (the files stay under 64 MB in all)
DUMP_BUDGET_ELEMS = 12 * 1024 * 1024


def _flatten_outputs(prefix, obj, out):
    """Nested state (dicts / lists of tensors and numbers) -> {dotted name:
    tensor or number}, in the state's own order; None leaves are dropped."""
    if obj is None:
        return
    if isinstance(obj, dict):
        for k, v in obj.items():
            _flatten_outputs(f"{prefix}.{k}" if prefix else str(k), v, out)
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            _flatten_outputs(f"{prefix}.{i}", v, out)
    elif torch.is_tensor(obj) or isinstance(obj, (bool, int, float)):
        out[prefix] = obj


def dump_outputs(out_dir, server, client_names, log, last_round):
    """Write what the last timed round handed back: per client, the upload
    state the server holds after the round's sync (trained weights, task
    token, sample count) and the round's training loss / accuracy.

    Tensors go out as float32, numbers as float64.  Every array gets the same
    share of DUMP_BUDGET_ELEMS; a larger one is reduced to a fixed seeded
    sample of its flattened (logical-order) elements, identical from run to
    run."""
    import numpy as np

    flat = {}
    for cname in client_names:
        _flatten_outputs(f"upload.{cname}", server.clients.get(cname), flat)
        rounds = log.records.get("data", {}).get(cname, {})
        for task, rec in rounds.get(str(last_round), {}).items():
            for key in ("tr_loss", "tr_acc"):
                if isinstance(rec, dict) and rec.get(key) is not None:
                    flat[f"train.{cname}.{task}.{key}"] = float(rec[key])
    if not flat:
        raise RuntimeError("--dump-outputs: the last round produced no outputs")

    os.makedirs(out_dir, exist_ok=True)
    cap = max(1, DUMP_BUDGET_ELEMS // len(flat))
    for name, value in flat.items():
        if torch.is_tensor(value):
            arr = value.detach().to(torch.float32).cpu().numpy().reshape(-1)
            if arr.size > cap:
                idx = np.random.default_rng(0).choice(arr.size, cap,
                                                      replace=False)
                arr = arr[np.sort(idx)]
            else:
                arr = arr.reshape(tuple(value.shape))
            arr = np.ascontiguousarray(arr, dtype=np.float32)
        else:
            arr = np.asarray(value, dtype=np.float64)
        np.save(os.path.join(out_dir, name.replace(os.sep, "_") + ".npy"), arr)


def build_configs(args, world_size, rank, work_dir):
    """`work_dir`: where this process's round log (and ckpts, when the audit
    trail is switched back on) go — a scratch directory, since neither the
    current directory nor the checkout need be writable."""
    h, w = (int(x) for x in args.img.split("x"))
    n_clients = max(args.gpus, world_size)
    common = {
        "datasets_dir": (f"synthetic://ids={args.ids},train={args.imgs_per_id},"
                         f"query=2,gallery=4,hw={h}x{w},"
                         f"idspace={min(4096, args.num_classes)}"),
        "checkpoints_dir": os.path.join(work_dir, "bench_ckpts"),
        "logs_dir": os.path.join(work_dir, "bench_logs"),
        "parallel": 1,
        "device": ["cpu" if args.cpu else "cuda:0"],
        "defaults": {},
    }
    exp = {
        "exp_name": "bench", "exp_method": args.method, "random_seed": 42,
        "exp_opts": {"comm_rounds": args.steps + args.warmup,
                     "val_interval": 0, "online_clients": n_clients,
                     "initial_validation": False,
                     "persist_comm_ckpts": False},
        "model_opts": {"name": args.model, "num_classes": args.num_classes,
                       "last_stride": 1, "neck": "bnneck",
                       "atten_default": 0.9, "lambda_l1": args.lambda_l1,
                       "lambda_k": args.lambda_k,
                       "fine_tuning": (["base.layers.3", "classifier"]
                                       if args.model.startswith("swin")
                                       else ["base.layer4", "classifier"])},
        "criterion_opts": {"name": "cross_entropy",
                           "num_classes": args.num_classes, "epsilon": 0.1},
        "optimizer_opts": {"name": "adam", "lr": 1e-3, "weight_decay": 1e-5},
        "scheduler_opts": {"name": "step_lr", "step_size": 5},
        "task_opts": {"sustain_rounds": 10 ** 9, "train_epochs": 1,
                      "augment_opts": {"level": "default", "img_size": [h, w],
                                       "norm_mean": [0.485, 0.456, 0.406],
                                       "norm_std": [0.229, 0.224, 0.225]},
                      "loader_opts": {"batch_size": args.batch,
                                      "num_workers": 0, "pin_memory": False,
                                      "persistent_workers": False,
                                      "multiprocessing_context": None}},
        "server": {"server_name": "server", "distance_calculate_step": 10,
                   "distance_calculate_decay": 0.8},
        "clients": [{"client_name": f"client-{i}",
                     "tasks": [f"task-{i}-0"]} for i in range(n_clients)],
    }
    return common, exp


def main():
    args = parse_args()
    from flreid_amd.parallel.comm import destroy_context, init_context
    from flreid_amd.runtime.builder import parser_clients, parser_server
    from flreid_amd.runtime.experiment import ExperimentStage
    from flreid_amd.runtime.log import ExperimentLog
    from flreid_amd.tools.utils import same_seeds

    ctx = init_context(device="cpu" if args.cpu else None)
    device_is_cuda = ctx.device.startswith("cuda")
    if device_is_cuda:
        from flreid_amd import ops
        if not ops.extension_available():
            raise RuntimeError(
                "flreid HIP extension not built — run "
                "`python -m flreid_amd.ops.build` before benchmarking")

    import shutil
    import tempfile
    work_dir = tempfile.mkdtemp(prefix=f"flreid_bench_r{ctx.rank}_")
    try:
        common, exp = build_configs(args, ctx.world_size, ctx.rank, work_dir)
        os.makedirs(common["logs_dir"], exist_ok=True)

        same_seeds(exp["random_seed"])
        stage = ExperimentStage(common, [exp], ctx=ctx)
        log = ExperimentLog(os.path.join(common["logs_dir"], "bench.json"))

        server = parser_server(exp, common)
        client_names = [c["client_name"] for c in exp["clients"]]
        owned = [i for i in range(len(client_names))
                 if ctx.owner_of(i) == ctx.rank]
        clients = parser_clients(exp, common, owned_indices=owned)
        by_name = {c.client_name: c for c in clients}
        if args.channels_last and device_is_cuda:
            for c in clients:
                # per-tensor conversion: methods with >4-D parameters (FedWeIT's
                # stacked knowledge base) break Module.to(channels_last)
                for m in c.model.net.modules():
                    for p in list(m.parameters(recurse=False)) + \
                            list(m.buffers(recurse=False)):
                        if p.dim() == 4:
                            p.data = p.data.to(memory_format=torch.channels_last)
                # the 7x7 stem stays NCHW: MIOpen's NHWC path falls back to a
                # naive kernel for it (measured 2.4 ms/call); the two layout
                # transposes around the stem cost microseconds
                stem = getattr(getattr(c.model.net, "base", None), "conv1", None)
                if stem is not None:
                    stem.weight.data = stem.weight.data.contiguous()

        def one_round(r):
            stage.process_one_round(r, server, by_name, client_names, exp, log)

        # images processed per round per client = the task's train split size
        imgs_per_client = args.ids * args.imgs_per_id
        n_clients = len(client_names)

        for r in range(1, args.warmup + 1):
            one_round(r)

        ctx.barrier()
        if device_is_cuda:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        for r in range(args.warmup + 1, args.warmup + args.steps + 1):
            one_round(r)
        ctx.barrier()
        if device_is_cuda:
            torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0

        # max over ranks
        elapsed = ctx.all_reduce_scalar(elapsed, op="max")

        if args.dump_outputs and ctx.is_rank0():
            dump_outputs(args.dump_outputs, server, client_names, log,
                         args.warmup + args.steps)

        # Rank-1 on the synthetic tasks (the BASELINE metric pairs throughput
        # with Rank-1) — measured OUTSIDE the timed region, --full runs only
        rank1 = None
        if args.full:
            rank1_sum = 0.0
            for client in clients:
                task = client.task_pipeline.get_task(0)
                cmc, _mAP, _rep = client.validate(
                    task_name=task["task_name"], query_loader=task["query_loader"],
                    gallery_loader=task["gallery_loaders"], device=stage.device)
                rank1_sum += float(cmc[0])
            rank1 = ctx.all_reduce_scalar(rank1_sum) / max(1, n_clients)

        if ctx.is_rank0():
            total_images = imgs_per_client * n_clients * args.steps
            value = total_images / elapsed
            result = {
                "metric": f"images/sec (whole node) per fed round, {args.method} {args.model}",
                "value": round(value, 2),
                "unit": "images/sec",
                "n_gpus": max(1, ctx.world_size),
                "steps": args.steps,
                "warmup": args.warmup,
                "ms_per_step": round(elapsed / args.steps * 1000, 2),
                "higher_is_better": True,
                "scaling": "weak",
                "vs_baseline": None,
                "dtype": "bf16" if device_is_cuda else "fp32",
                "data": "synthetic",
                "config": {
                    "model": f"{args.model}-{args.method}",
                    "global_batch": args.batch * n_clients,
                    "img": args.img,
                    "images_per_round_per_client": imgs_per_client,
                    "num_classes": args.num_classes,
                    "lambda_k": args.lambda_k,
                    "rehearsal_set": (f"{args.lambda_k} exemplar budget + task "
                                      f"(m={-(-args.lambda_k // args.ids)}/id)"),
                    "parallelism": f"fed-dp{max(1, ctx.world_size)} (1 client/GPU)",
                },
            }
            if rank1 is not None:
                result["rank1"] = round(rank1, 4)
            print(json.dumps(result))
        destroy_context()
    finally:
        shutil.rmtree(work_dir, ignore_errors=True)


if __name__ == "__main__":
    main()
