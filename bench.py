#!/usr/bin/env python3
"""Headline benchmark: Notebook-CR reconciles/sec + create→Ready latency at N GPU pods.

BASELINE.json metric: "Notebook-CR reconciles/sec + p50 pod-Ready latency at 1/2/4/8 GPU
pods"; configs 2/3 ("1 Notebook pod requesting amd.com/gpu=1 on one MI355X", "8
concurrent Notebook CRs, one per MI355X").

One *step* is one full notebook lifecycle per rank (one rank per MI355X of the node):

  create a Notebook CR (``amd.com/gpu: 1``, PyTorch-ROCm image, odh auth/route path) →
  mutating webhook → kf + odh reconcilers → StatefulSet → scheduler + first-free
  ``amd.com/gpu`` allocation → kubelet → pod Ready → Notebook status Ready → delete →
  finalizers and owned objects gone.

The control plane is the shipped process(es) (``--arch sharded``: ``cmd/control_plane.py
--shard r`` per rank; ``--arch unsharded``: one ``cmd/kf_manager.py`` + one
``cmd/odh_manager.py`` for every rank's notebooks).  The Ready path is the default
deployment's: no start-up probe (``amd.com/gpu-probe`` is opt-in).

A plain run does what the headline needs and no more: it sets up, warms up, times the K
steps and prints the result line (``--dump-outputs DIR``: and writes what the last timed step
produced).  ``--full`` adds everything measured beside it, untimed: the in-process
(envtest-style) figure, the RCCL check, a few probe notebooks (``gpu_probe_init_container``),
the ``burst``, ``resident`` and ``storage`` blocks and the BASELINE configs #2-#5.

``value`` = reconciles completed by the notebook controllers inside the K timed steps ÷ the
timed wall time (whole job).  Weak scaling: N notebooks in flight on N GPUs.  The figure
that matters for users leads the JSON: ``notebooks_ready_per_s`` and p50/p95 create→Ready.

Launch (driver contract): ``python bench.py --gpus N --steps K --warmup W`` or under
``torch.distributed.run`` with one rank per GPU.  Data: synthetic Notebook CRs; no
images are pulled (the kubelet stand-in starts no container process by default).
"""

from __future__ import annotations

import argparse
import asyncio
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

METRIC = "Notebook-CR reconciles/sec + p50 pod-Ready latency at 1/2/4/8 GPU pods"
MODEL = "kubeflow.org/v1 Notebook (amd.com/gpu=1, PyTorch-ROCm image) on 8xMI355X node"


def parse(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=int(os.environ.get("WORLD_SIZE", "1")))
    p.add_argument("--steps", type=int, default=300)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--probe-sample", type=int, default=4,
                   help="after the timed region: notebooks per rank with the odh-gpu-probe init container (needs a GPU)")
    p.add_argument("--probe-gap-s", type=float, default=0.5,
                   help="pause before each probe notebook: a GPU process that exited within ~0.15 s "
                        "still holds the next one's HIP init in the kernel driver's teardown")
    p.add_argument("--no-gpu-probe", action="store_true", help="skip the start-up probe sample (CPU dev runs)")
    p.add_argument("--no-odh", action="store_true", help="kf controller only (no webhook / odh reconciler)")
    p.add_argument("--reference-emulation", action="store_true",
                   help="reproduce the reference's serialising behaviour (1 worker, blocking lock removal)")
    p.add_argument("--transport", choices=("inprocess", "http", "native"), default="inprocess",
                   help="managers share the store (inprocess) or talk REST/watch to the apiserver (http)")
    p.add_argument("--arch", choices=("auto", "inprocess", "sharded", "unsharded"), default="auto",
                   help="sharded: one control-plane shard process per rank (overlay mi355x-sharded; the headline "
                        "at every N); unsharded: one kf + one odh manager process for all ranks (overlay mi355x, "
                        "the reference topology); inprocess: one process, controllers share the store "
                        "(envtest-style); auto: sharded, plus the in-process figure as a secondary field at N=1")
    p.add_argument("--no-inprocess-baseline", action="store_true",
                   help="N=1 auto: skip the extra in-process (envtest-style) measurement")
    p.add_argument("--single-process-shard", action="store_true",
                   help="sharded: each shard as ONE control-plane process (kf + odh + webhook) instead of the "
                        "deployed kf | odh | webhook processes (A/B measurements)")
    p.add_argument("--workers", type=int, default=1,
                   help="unsharded: --workers of the kf and odh managers (namespace-partitioned worker processes)")
    p.add_argument("--webhook-in-odh", action="store_true",
                   help="sharded: each shard's webhook in its odh process (round 3-4's shard pod) instead of a "
                        "process of its own (A/B measurements)")
    p.add_argument("--cache-configmaps", action="store_true",
                   help="unsharded: the odh manager caches ConfigMap/Secret data (--cache-configmaps-secrets=true) "
                        "instead of the reference's live, data-stripped reads")
    p.add_argument("--kf-split-workers", action="store_true",
                   help="unsharded with --workers: the kf manager's --split-workers (per namespace set a notebook "
                        "reconciler process and a culler + event re-emitter process)")
    p.add_argument("--webhook-replicas", type=int, default=1,
                   help="unsharded with --workers: --webhook-replicas of the odh manager (webhook processes sharing "
                        "the port)")
    p.add_argument("--namespaces-per-rank", type=int, default=1,
                   help="each rank drives its notebooks round-robin over M user namespaces (bench-r-j); sharded: "
                        "created unlabelled and assigned to shards by the shipped NamespaceShardAssigner "
                        "(crc32(name) %% N), so a shard serves the namespaces that hash to it, whichever rank "
                        "drives them — per-shard notebooks, notebooks/s and CPU are reported")
    p.add_argument("--cluster-wide-watches", action="store_true",
                   help="control-plane processes watch each kind once, cluster-wide, filtering namespaces "
                        "themselves, instead of one watch per served namespace per kind (A/B at many namespaces)")
    p.add_argument("--assign-policy", choices=("hash", "balanced"), default="hash",
                   help="--namespaces-per-rank, sharded: the NamespaceShardAssigner policy (hash: crc32 %% N; "
                        "balanced: the shard owning the fewest namespaces, as overlay mi355x-sharded deploys it)")
    p.add_argument("--burst", type=int, default=32,
                   help="after the timed window: this many notebooks created at once (open loop), split over the "
                        "ranks — time to all Ready, notebooks/s at saturation, admission latency (0: skip)")
    p.add_argument("--platform-workers", type=int, default=0,
                   help="node platform: StatefulSet-controller and kubelet stand-in processes (0: one per two ranks)")
    p.add_argument("--burst-rounds", type=int, default=2,
                   help="bursts in a row; the last is reported (the first warms the apiserver's webhook "
                        "connections, as on a running cluster)")
    p.add_argument("--openshift-pull-secret-ms", type=float, default=-1.0,
                   help=">= 0: an OpenShift-like cluster — the OpenShift APIs served and every ServiceAccount's "
                        "dockercfg pull secret added this many ms after it appears (the reference's lock waits "
                        "for it); default: vanilla Kubernetes")
    p.add_argument("--write-latency-ms", type=float, default=0.0,
                   help="etcd-like storage latency the native apiserver adds to every write")
    p.add_argument("--no-configs", action="store_true",
                   help="skip the BASELINE configs #2-#5 sample that follows the N=1 run (real workbench "
                        "processes, the webhook path across 8, GPU-busy culling across 8)")
    p.add_argument("--no-culling", action="store_true",
                   help="run the control plane without the culler (the MI355X overlays ship it on: "
                        "ENABLE_CULLING=true, CULLING_ACTIVITY_SOURCE=combined)")
    p.add_argument("--culler-in-kf", action="store_true",
                   help="sharded: the culler in the kf process (the reference's manager layout) instead of a process "
                        "of its own (A/B measurements)")
    p.add_argument("--culling-period", type=float, default=1.0,
                   help="the culler's check period in seconds (IDLENESS_CHECK_PERIOD_SECONDS; the overlays' "
                        "is 60): every resident notebook is checked, and its Notebook written, once per period")
    p.add_argument("--culler-stamp-every", type=int, default=10,
                   help="CULL_CHECK_STAMP_EVERY of the culler (the MI355X overlays' 10; 1: the reference's write "
                        "of the check stamp on every check)")
    p.add_argument("--resident", type=int, default=256,
                   help="after the window: this many notebooks created and left running with the culler on "
                        "(the reference's loadtest scenario); reported: the control plane's cost at rest and "
                        "new notebooks' create->Ready on top of them (0: skip)")
    p.add_argument("--resident-window", type=float, default=3.0, help="seconds measured at rest")
    p.add_argument("--resident-steps", type=int, default=20,
                   help="closed-loop lifecycles per rank on top of the resident population")
    p.add_argument("--resident-warmup", type=int, default=10,
                   help="untimed lifecycles per rank before those (as --warmup before the window)")
    p.add_argument("--storage-steps", type=int, default=20,
                   help="after the window: closed-loop lifecycles per rank with --storage-ms of etcd-like latency "
                        "on every apiserver write (reported in 'storage'; 0: skip)")
    p.add_argument("--storage-ms", type=float, default=2.0, help="the storage block's per-write latency")
    p.add_argument("--json-out", default=None)
    p.add_argument("--full", action="store_true",
                   help="everything beside the headline too: the in-process (envtest-style) figure, the RCCL "
                        "check, the start-up probe sample, the burst, resident and storage blocks and the "
                        "BASELINE configs #2-#5 (each still has its own switch); without it a run sets up, "
                        "warms up, times the steps and prints the result line")
    p.add_argument("--dump-outputs", default=None, metavar="DIR",
                   help="after the timed steps: what the last timed step produced (the Ready Notebook and its "
                        "pod, see lifecycle_outputs) as DIR/<name>.npy, float64")
    args = p.parse_args(argv)
    if not args.full:  # the headline alone: nothing that takes a run (or a block after the window) of its own
        args.no_inprocess_baseline = args.no_configs = args.no_gpu_probe = True
        args.burst = args.resident = args.storage_steps = 0
    return args


def pct(xs, q):
    if not xs:
        return None
    xs = sorted(xs)
    k = (len(xs) - 1) * q
    lo = int(k)
    hi = min(lo + 1, len(xs) - 1)
    return xs[lo] + (xs[hi] - xs[lo]) * (k - lo)


# set by the apiserver or by the clock, different in every run: left out of the dumped outputs
VOLATILE_KEYS = frozenset((
    "uid", "resourceVersion", "creationTimestamp", "deletionTimestamp", "managedFields", "generation", "selfLink",
    "startTime", "startedAt", "finishedAt", "lastTransitionTime", "lastProbeTime", "lastHeartbeatTime", "containerID",
    "observedGeneration"))


def _stable(o):
    """``o`` without the fields of VOLATILE_KEYS, keys sorted (lists keep their order: it is
    part of what the controllers wrote)."""
    if isinstance(o, dict):
        return {k: _stable(v) for k, v in sorted(o.items()) if k not in VOLATILE_KEYS}
    if isinstance(o, list):
        return [_stable(v) for v in o]
    return o


def _json_bytes(o):
    import numpy as np

    text = json.dumps(_stable(o), sort_keys=True, separators=(",", ":"))
    return np.frombuffer(text.encode(), dtype=np.uint8).astype(np.float64)


def lifecycle_outputs(notebook, pod) -> dict:
    """What a caller of one timed step receives — the Notebook as it turned Ready and its pod —
    as float64 arrays, the same from run to run (names and namespaces follow from the step
    number; VOLATILE_KEYS and the Notebook's annotations, where the culler keeps its clock,
    are left out):

    * ``notebook_summary``: readyReplicas, Ready condition True, conditions, containers and
      volumes of the (mutated) pod template;
    * ``pod_summary``: Ready condition True, phase Running, containers, init containers,
      volumes, ``amd.com/gpu`` limit of the first container, the allocated GPU indices
      (``amd.com/gpu-ids``, padded with -1 to the node's 8);
    * ``notebook_json`` / ``pod_json``: the UTF-8 bytes of the canonical JSON of the Notebook's
      labels, spec and status and of the pod's labels, annotations, spec and status, so that
      two builds can be compared field for field (``bytes(a.astype('uint8'))`` reads it back)."""
    import numpy as np

    nb, pod = notebook or {}, pod or {}

    def cond(o, typ):
        return float(any(c.get("type") == typ and c.get("status") == "True"
                         for c in (o.get("status") or {}).get("conditions") or []))

    tmpl = (((nb.get("spec") or {}).get("template") or {}).get("spec") or {})
    nst = nb.get("status") or {}
    pspec, pst, pmeta = pod.get("spec") or {}, pod.get("status") or {}, pod.get("metadata") or {}
    ctrs = pspec.get("containers") or []
    limit = ((ctrs[0].get("resources") or {}).get("limits") or {}).get("amd.com/gpu", 0) if ctrs else 0
    ids = [float(x) for x in str((pmeta.get("annotations") or {}).get("amd.com/gpu-ids", "")).split(",")
           if x.strip().lstrip("-").isdigit()][:8]
    nmeta = nb.get("metadata") or {}
    return {
        "notebook_summary": np.array([float(nst.get("readyReplicas") or 0), cond(nb, "Ready"),
                                      float(len(nst.get("conditions") or [])), float(len(tmpl.get("containers") or [])),
                                      float(len(tmpl.get("volumes") or []))], dtype=np.float64),
        "pod_summary": np.array([cond(pod, "Ready"), float(pst.get("phase") == "Running"), float(len(ctrs)),
                                 float(len(pspec.get("initContainers") or [])), float(len(pspec.get("volumes") or [])),
                                 float(limit), *ids, *([-1.0] * (8 - len(ids)))], dtype=np.float64),
        "notebook_json": _json_bytes({"labels": nmeta.get("labels"), "spec": nb.get("spec"), "status": nst}),
        "pod_json": _json_bytes({"labels": pmeta.get("labels"), "annotations": pmeta.get("annotations"),
                                 "spec": pspec, "status": pst}),
    }


def dump_outputs(directory: str, per_rank: list) -> None:
    """``DIR/<name>.npy``: the last timed step's outputs, one rank's after the other's."""
    import numpy as np

    os.makedirs(directory, exist_ok=True)
    for name in sorted({k for o in per_rank for k in o}):
        parts = [np.asarray(o[name], dtype=np.float64) for o in per_rank if name in o]
        np.save(os.path.join(directory, f"{name}.npy"), np.concatenate(parts) if parts else np.zeros(0))


async def run_local(args, n_gpus: int) -> dict:
    from odh_kubeflow_amd.testing.cluster import ClusterConfig, LocalCluster
    from odh_kubeflow_amd.models import kinds
    from odh_kubeflow_amd.models.notebook import notebook

    use_odh = not args.no_odh and _odh_available()
    cfg = ClusterConfig(gpus_per_node=8, odh=use_odh, webhook=use_odh,
                        reference_emulation=args.reference_emulation, transport=args.transport,
                        env={"SET_PIPELINE_RBAC": "false", "SET_PIPELINE_SECRET": "false"})
    lat_ms, teardown_ms = [], []
    recon = 0
    last = {}  # the last timed step's Ready notebooks and their pods (--dump-outputs)
    async with LocalCluster(cfg) as cl:
        await cl.ensure_namespace("bench")
        step_id = 0

        async def one_step(timed: bool):
            nonlocal step_id
            step_id += 1
            names = [f"nb-s{step_id}-g{i}" for i in range(n_gpus)]
            ann = {"notebooks.opendatahub.io/inject-auth": "true"} if use_odh else None
            t0 = {}
            ready_at = {}

            async def create(nm):
                t0[nm] = time.perf_counter()
                await cl.admin.create(notebook(nm, "bench", image="rocm/pytorch:rocm7.0_ubuntu22.04_py3.10_pytorch_2.10",
                                               gpus=1, annotations=ann))

            await asyncio.gather(*(create(nm) for nm in names))
            pending = set(names)
            deadline = time.monotonic() + 120
            while pending and time.monotonic() < deadline:
                for nm in list(pending):
                    if cl.notebook_ready(nm, "bench"):
                        ready_at[nm] = time.perf_counter()
                        pending.discard(nm)
                if pending:
                    await asyncio.sleep(0.0005)
            if pending:
                raise RuntimeError(f"notebooks not Ready: {sorted(pending)}")
            if timed and args.dump_outputs and step_id == args.warmup + args.steps:
                last.update({nm: (cl.store.peek(kinds.NOTEBOOK, nm, "bench"), cl.store.peek(kinds.POD, f"{nm}-0", "bench"))
                             for nm in names})
            t_del = time.perf_counter()
            await asyncio.gather(*(cl.admin.delete(kinds.NOTEBOOK, nm, "bench") for nm in names))
            ok = await cl.wait_for(lambda: all(cl.store.peek(kinds.NOTEBOOK, nm, "bench") is None and
                                               cl.store.peek(kinds.POD, f"{nm}-0", "bench") is None
                                               for nm in names), 60, 0.0005)
            if not ok:
                left = [(k, o) for nm in names for k, o in ((kinds.NOTEBOOK, nm), (kinds.POD, f"{nm}-0"))
                        if cl.store.peek(k, o, "bench") is not None]
                raise RuntimeError(f"teardown did not finish: {[cl.store.peek(k, o, 'bench') for k, o in left]}")
            if timed:
                lat_ms.extend((ready_at[nm] - t0[nm]) * 1e3 for nm in names)
                teardown_ms.append((time.perf_counter() - t_del) * 1e3)

        for _ in range(args.warmup):
            await one_step(False)
        await cl.settle(5)
        from odh_kubeflow_amd.utils import gctune

        gctune.tune()  # start-up heap out of the cyclic collector's reach (see utils/gctune.py)
        r0 = cl.reconcile_count()
        b0 = cl.reconcile_breakdown()
        t_start = time.perf_counter()
        for _ in range(args.steps):
            await one_step(True)
        # the window ends with the last step; its trailing reconciles fall outside, as the
        # warm-up's did at the start (under continuous load they overlap the next step)
        elapsed = time.perf_counter() - t_start
        recon = cl.reconcile_count() - r0
        await cl.settle(5)  # untimed: the per-lifecycle count includes them
        breakdown = breakdown_delta(b0, cl.reconcile_breakdown())
    return {"elapsed": elapsed, "reconciles": recon, "lat_ms": lat_ms, "odh": use_odh,
            "teardown_ms": teardown_ms, "breakdown": breakdown,
            "outputs": [lifecycle_outputs(nb, pod) for _nm, (nb, pod) in sorted(last.items())]}


def breakdown_delta(b0: dict, b1: dict) -> dict:
    """Reconciles per controller and triggering watch kind between two snapshots."""
    out = {}
    for ctrl, trig in b1.items():
        d = {k: v - b0.get(ctrl, {}).get(k, 0) for k, v in trig.items()}
        d = {k: v for k, v in d.items() if v}
        if d:
            out[ctrl] = d
    return out


def merge_breakdowns(parts) -> dict:
    out: dict = {}
    for b in parts:
        for ctrl, trig in (b or {}).items():
            o = out.setdefault(ctrl, {})
            for k, v in trig.items():
                o[k] = o.get(k, 0) + v
    return out


def _odh_available() -> bool:
    try:
        import odh_kubeflow_amd.controllers.odh.reconciler  # noqa: F401
        import odh_kubeflow_amd.webhook.notebook_webhook  # noqa: F401
        return True
    except ImportError:
        return False


def _compile_bytecode() -> None:
    """Byte-compile the package before anything is timed, as a container image build does
    (pip writes the .pyc files at install): a fresh checkout has none, so every process of the
    control plane and the node platform would otherwise compile its modules — and those first
    imported inside the timed window, within it.  A no-op once they exist."""
    import compileall

    try:
        root = os.path.dirname(os.path.abspath(__file__))
        compileall.compile_dir(os.path.join(root, "odh_kubeflow_amd"), quiet=2)  # in this process: no pool
    except Exception:  # noqa: BLE001 — a read-only tree: the processes compile in memory as before
        pass


def main(argv=None):
    args = parse(argv)
    rank = int(os.environ.get("RANK", "0"))
    if int(os.environ.get("LOCAL_RANK", "0")) == 0:
        _compile_bytecode()
    n = args.gpus
    if args.arch in ("auto", "sharded", "unsharded"):
        # production architecture at every N (one control-plane shard per MI355X rank against
        # the native apiserver), so the 1/2/4/8 curve compares like with like
        inproc = None
        if n == 1 and args.arch == "auto" and not args.no_inprocess_baseline:
            # BASELINE config #1 (envtest-style: controllers share the in-process store)
            inproc = _run_inprocess(args, n)
        _single_rank_env()
        from odh_kubeflow_amd.parallel.bench_dist import measure

        out = measure(args)
        if out is not None and inproc is not None:
            out["inprocess_n1"] = {k: inproc.get(k) for k in (
                "value", "ms_per_step", "p50_ready_ms", "p95_ready_ms", "notebooks_ready_per_s",
                "reconciles_per_notebook", "p50_teardown_ms")}
    else:
        out = _run_inprocess(args, n, dump=True)
    if rank == 0 and out is not None and n == 1 and not args.no_configs:
        out["configs"] = run_configs(args)
    if rank == 0 and out is not None:
        print(json.dumps(out), flush=True)
        if args.json_out:
            with open(args.json_out, "w") as f:
                json.dump(out, f, indent=1)
    return 0


CONFIG_RUNS = (
    # (key, BASELINE config, command, time limit s, needs the GPU)
    ("real_pods", "#2/#3: 1 and 8 notebooks whose container is a real PyTorch-ROCm workbench process on the MI355X",
     ["tools/bench_real_pods.py", "--notebooks", "1,8", "--repeats", "1", "--gpu-probe", "off"], 90, True),
    ("webhook_8", "#4: odh webhook path (kube-rbac-proxy sidecar + Istio VirtualService + HTTPRoute) across 8",
     ["tools/bench_webhook.py", "--rounds", "3", "--warmup", "1"], 60, False),
    ("culling_8", "#5: idle culling on amdgpu busy counters across 8 GPU notebooks, under MFMA load",
     ["tools/bench_culling.py", "--idle-s", "1", "--period-s", "0.2", "--load-s", "3"], 90, True),
)


def run_configs(args) -> dict:
    """BASELINE configs #2-#5, untimed, after the headline run (N=1 only): each tool runs as a
    child process with a short setting and its JSON result is carried in the bench line, so the
    driver observes them.  Without a GPU the real-pod sample is skipped and culling runs on a
    synthetic sysfs tree."""
    import subprocess

    try:
        import torch

        gpu = torch.cuda.device_count() > 0
    except Exception:  # noqa: BLE001
        gpu = False
    here = os.path.dirname(os.path.abspath(__file__))
    out = {}
    for key, what, cmd, limit, needs_gpu in CONFIG_RUNS:
        if needs_gpu and not gpu:
            if key != "culling_8":
                out[key] = {"config": what, "skipped": "no GPU visible"}
                continue
            cmd = [*cmd, "--cpu"]
        t0 = time.perf_counter()
        try:
            r = subprocess.run([sys.executable, *cmd], cwd=here, capture_output=True, text=True, timeout=limit)
            lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
            if r.returncode != 0 or not lines:
                out[key] = {"config": what, "error": f"rc={r.returncode}: {(r.stderr or r.stdout)[-400:]}"}
                continue
            docs = [json.loads(ln) for ln in lines]
            for d in docs:  # the per-notebook detail stays in the tool's own output
                d.pop("per_notebook", None)
                d.pop("device_ids", None)
            out[key] = {"config": what, "result": docs if len(docs) > 1 else docs[0]}
        except subprocess.TimeoutExpired:
            out[key] = {"config": what, "error": f"timed out after {limit} s"}
        out[key]["wall_s"] = round(time.perf_counter() - t0, 2)
        out[key]["command"] = " ".join(["python", *cmd])
    return out


def _run_inprocess(args, n: int, dump: bool = False) -> dict:
    """One process: every controller, the webhook and the kubelet stand-ins share the object store."""
    res = asyncio.run(run_local(args, n))
    if dump and args.dump_outputs:
        dump_outputs(args.dump_outputs, res["outputs"])
    out = report(args, n, res)
    out["config"]["architecture"] = "inprocess"
    return out


def _single_rank_env() -> None:
    if "MASTER_ADDR" not in os.environ:  # single rank without a launcher
        import socket

        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(s.getsockname()[1]),
                              RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")


def report(args, n, res) -> dict:
    el = res["elapsed"]
    lat = res["lat_ms"]
    nbs = max(1, len(lat))
    lifecycle = sum(sum(t.values()) for t in (res.get("breakdown") or {}).values()) or res["reconciles"]
    out = {
        "metric": METRIC,
        "value": round(res["reconciles"] / el, 2) if el > 0 else None,
        "unit": "reconciles/s",
        "notebooks_ready_per_s": round(len(lat) / el, 3) if el > 0 else None,
        "p50_ready_ms": round(pct(lat, 0.5), 3) if lat else None,
        "p95_ready_ms": round(pct(lat, 0.95), 3) if lat else None,
        "max_ready_ms": round(max(lat), 3) if lat else None,
        "n_gpus": n, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(el / max(1, args.steps) * 1e3, 3),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        # a control plane: no tensor compute in the timed region (the GPU work is the opt-in
        # start-up probe, reported in gpu_probe_init_container)
        "dtype": "n/a", "data": "synthetic",
        "config": {"model": MODEL, "notebooks_per_step": n,
                   "parallelism": f"controllers max_concurrent=8 x{n}", "odh_webhook_path": res.get("odh", False)},
        "reconciles_in_window": res["reconciles"],
        "reconciles_per_notebook": round(lifecycle / nbs, 2),
    }
    if res.get("breakdown"):
        # per controller: reconciles per notebook lifecycle, split by the watch kind that queued them
        out["reconciles_per_notebook_by_controller"] = {
            ctrl: {"total": round(sum(t.values()) / nbs, 2),
                   "by_trigger": {k: round(v / nbs, 2) for k, v in sorted(t.items(), key=lambda kv: -kv[1])}}
            for ctrl, t in sorted(res["breakdown"].items())}
    if getattr(args, "reference_emulation", False):
        # not the framework's numbers: the reference's serialising odh path, same harness
        out["config"]["reference_emulation"] = True
        out["config"]["parallelism"] = f"reference emulation x{n} (1 odh worker, blocking lock removal)"
    if res.get("teardown_ms"):
        out["p50_teardown_ms"] = round(pct(res["teardown_ms"], 0.5), 3)
    return out


if __name__ == "__main__":
    sys.exit(main())
