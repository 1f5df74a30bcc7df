#!/usr/bin/env python3
"""Benchmark of the MI355X peptide-WAE training step (BASELINE.json metric: peptide-seq/s per WAE step).

  python bench.py --gpus N --steps K --warmup W          (N>1: launched by torch.distributed.run, one rank per GPU)

A step = one full train_vae iteration on one synthetic batch already resident in HBM: encoder + reparameterisation +
teacher-forced decoder, recon CE + KL + full-kernel MMD + random-feature MMD, backward, flat-gradient all-reduce
(N>1), global-norm clip + Adam; all random draws (eps, c, both dropout masks, z_prior) are generated on the device
inside the step.  Prints ONE JSON line (rank 0) with the `roofline` and `cpu_baseline` objects described in DESIGN.md.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(ROOT, "controlled-peptide-generation_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

PEAK_F32_MFMA_TFLOPS = 157.3   # MI355X f32-input MFMA = f32 vector peak (MI355X_MICROARCH.md, chip-level parameters)
PEAK_BF16_MFMA_TFLOPS = 2500.0  # dense bf16 MFMA peak (same guide)
# Kernels on the split engine compute an f32-grade product as SIX bf16 MFMAs on 3-way split operands: the best f32-grade rate
# that pipe can give is the bf16 peak / 6.  Exact kernels (v_mfma_f32_16x16x4_f32) are priced against the f32 MFMA peak.
PEAK_SPLIT_TFLOPS = PEAK_BF16_MFMA_TFLOPS / 6.0
PEAK_PAIR_TFLOPS = PEAK_BF16_MFMA_TFLOPS / 3.0   # f32-grade on f16 pairs: three f16 MFMAs (same rate as bf16) per block (csrc/gemm_core.h)
HBM_PEAK_GBS = 8000.0
# HBM bytes per launch from PMC counters (FETCH_SIZE / WRITE_SIZE in KB, separate rocprofv3 passes, tools/pmc_run.sh +
# tools/pmc_summary.py --json): counters cannot be collected from inside this script, so the per-kernel means of the
# committed profile are looked up BY THE KERNEL NAME THE LAUNCHER REPORTS - a tile-policy change yields null, not a stale
# number.  (2*FETCH + WRITE)*1024: the gfx950 read-side correction of MI355X_MICROARCH.md, HBM section.
def _pmc_json():
    """The newest committed PMC profile (profiles/rNN_pmc.json) - pmc_traffic() only trusts it when its source fingerprint matches."""
    import glob
    c = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_pmc.json")))
    return c[-1] if c else os.path.join(ROOT, "profiles", "r05_pmc.json")


PMC_JSON = _pmc_json()


def csrc_fingerprint():
    """sha256 over the kernel sources (csrc/*.hip, *.h, sorted by name): what a PMC profile must have been taken from for its
    per-kernel byte counts to describe the kernels this run launches (the GPU box has no .git, so not a commit id)."""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(PKG, "csrc")
    for fn in sorted(os.listdir(d)):
        if fn.endswith((".hip", ".h")):
            h.update(fn.encode())
            h.update(open(os.path.join(d, fn), "rb").read())
    return h.hexdigest()[:16]


def pmc_traffic(kernel, grid=None):
    """HBM bytes per launch of `kernel` from the committed PMC profile - only when that profile was taken from THESE kernel
    sources (its "_csrc_sha256_16" stamp equals csrc_fingerprint()); otherwise null.  grid (work-items of the launch): picks the row of
    that launch shape where one instantiation serves several (tools/pmc_summary.py: "name @grid=N")."""
    try:
        d = json.load(open(PMC_JSON))
    except (OSError, ValueError):
        return None
    if d.get("_csrc_sha256_16") != csrc_fingerprint():
        return None
    # (rocprofv3 prints gemm_kernel's trailing bf16-operand template argument, the launcher's name query does not)
    r = (d.get("%s @grid=%d" % (kernel, grid)) if grid else None) or d.get(kernel) or d.get(kernel[:-1] + ", false>") or d.get(kernel[:-1] + ", true>")
    if not r or "FETCH_SIZE" not in r or "WRITE_SIZE" not in r:
        return None
    return (2.0 * r["FETCH_SIZE"] + r["WRITE_SIZE"]) * 1024.0


def profiled_launches():
    """(kernel launches per eager training step, of which torch / runtime glue) from the rocprofv3 kernel trace of the committed
    profile - when it was taken from these kernel sources; else (None, None)."""
    try:
        d = json.load(open(PMC_JSON))
    except (OSError, ValueError):
        return None, None
    if d.get("_csrc_sha256_16") != csrc_fingerprint():
        return None, None
    return d.get("_launches_per_step"), d.get("_torch_glue_launches_per_step")


def _cname(fn, *args):
    import ctypes
    from cpg import lib
    buf = ctypes.create_string_buffer(256)
    getattr(lib().dll, fn)(*args, buf, 256)
    return buf.value.decode()


def family_bytes(family, dims, bf16_gates):
    """ALGORITHMIC HBM bytes of one launch of a recurrent kernel family (DESIGN.md section 6 states the per-element figures): what the
    launch must move if every operand crossed HBM exactly once.  Per state element (one of B x H per direction and time step):
      forward   writes h (4) + the saved gates r, z, n, W_hn h + b_hn (4 x 4, or 4 x 2 as bf16) - state exchange stays in L2;
      backward  reads the saved gates (16 / 8), h_prev (4), the carry z (.) dH (4), the external gradient (4: decoder only) and
                writes dG (16) + the next carry (4);
      dW_hh     reads dG's hidden-side columns (12) and h_prev (4) once.  LSTM: four gate columns -> dG 16, gates + cell state.
    All-T planes form of the BPTT chain (dims["ap"], round 5): the backward step writes the three recurrent blocks ONLY as kept f16-pair
    planes (12) + dn_pre (4) + the state planes (4) + the carry (4) = 24 in place of 16 + 4 (the f32 dG AND the ping-pong planes before:
    32 by the counters); dW_hh reads the planes (12 + 4): the same bytes, no conversion."""
    T, B, H, nd = dims["T"], dims["B"], dims["H"], dims["ndir"]
    ap = bool(dims.get("ap"))
    g = 8 if bf16_gates else 16
    el = float(B) * H
    if family == "fwd_persist":
        return T * el * (4 + g)
    if family == "fwd_step":
        return nd * el * (4 + 4 + g)
    if family == "bwd_step":
        return nd * el * (g + 4 + 4 + (4 if nd == 1 else 0) + (20 if ap else 16) + 4)
    if family in ("wgrad_hh", "lstm_wgrad_hh"):
        return T * el * ((12 if family == "wgrad_hh" else 16) + 4)
    if family == "lstm_fwd_persist":
        return T * el * (4 + 4 + 16)
    if family == "lstm_fwd_step":
        return el * (4 + 4 + 4 + 4 + 16)
    if family == "lstm_bwd_step":
        return nd * el * (16 + 4 + 4 + 4 + 4 + 16 + 4 + 4)
    return None


def family_roofline(family, dims, avg_us, launches):
    """Roofline object of one kernel family of the step (names and product form come from the launcher).  Both roofs are priced -
    the matrix pipe the kernel uses and HBM on the family's algorithmic bytes - and `bound` / `frac` name the BINDING one (the
    larger fraction): in the bf16 compute mode the recurrent kernels sit at 8-13 % of the bf16 MFMA peak and are bound by their
    bytes, not by the pipe (round-3 verdict: the line used to print bound "mfma", peak 2500 for them)."""
    from cpg import lib
    T, B, H, nd = dims["T"], dims["B"], dims["H"], dims["ndir"]
    L = lib().dll
    bf16 = L.cpg_get_compute_mode() == 1
    if family == "fwd_persist":
        kernel, flops = _cname("cpg_gru_persistent_kernel_name", H), T * 2.0 * B * H * 3 * H
        split = {1: 2, 2: 3, 3: 1}[int(kernel.split("<")[1].split(",")[0])]   # planes of the kernel: 1 bf16 mode, 2 f16 pair, 3 bf16 triple
    elif family == "fwd_step":
        kernel, split = _cname("cpg_gru_step_kernel_name", 0, B, H, nd, 0), L.cpg_gru_step_kernel_is_split(0, B, H, nd, 0)
        flops = nd * 2.0 * B * H * 3 * H
    elif family == "bwd_step":
        kernel, split = _cname("cpg_gru_step_kernel_name", 1, B, H, nd, 1), L.cpg_gru_step_kernel_is_split(1, B, H, nd, 1)
        flops = nd * 2.0 * B * 3 * H * H
    elif family == "wgrad_hh" and dims.get("ap"):
        # all-T planes form (cpg_gru_wgrad_hh_ap -> csrc/pair_tn.h): both operands f16-pair planes in memory, three f16 MFMAs per block
        # (bf16 compute mode: the same loop on one bf16 plane per operand - its bf16 gate gradients and a bf16 copy of the states)
        kernel, flops, split = ("pair_tn_kernel<2, 2, 2, 0, 0, 1>" if bf16 else "pair_tn_kernel<2, 2, 2, 0, 0, 2>"), 2.0 * 3 * H * H * T * B, (2 if bf16 else 3)
    elif family == "wgrad_hh":
        pairs = int(L.cpg_gru_bwd_pair_bytes(B, H, 1) > 0)   # the f16-pair BPTT hands its column exponents to the product
        kernel, flops = _cname("cpg_gemm_tn_kernel_name", T * B, 3 * H, H, pairs), 2.0 * 3 * H * H * T * B
        split = 2 if kernel.endswith(", 1>") else 3 if kernel.endswith(", 8>") else 1
    elif family == "lstm_fwd_persist":
        kernel, flops = _cname("cpg_lstm_persistent_kernel_name", B, H), T * 2.0 * B * H * 4 * H
        split = {1: 2, 2: 3, 3: 1}[int(kernel.split("<")[1].split(",")[0])]
    elif family in ("lstm_fwd_step", "lstm_bwd_step"):   # LSTM extension: four gates
        kind = 0 if family == "lstm_fwd_step" else 1
        kernel, split = _cname("cpg_lstm_step_kernel_name", kind, B * nd, H), L.cpg_lstm_step_kernel_is_split(kind, B, H)
        flops = nd * 2.0 * B * H * 4 * H
    elif family == "lstm_wgrad_hh" and dims.get("ap"):   # all-T planes form of the LSTM extension (cpg_lstm_wgrad_hh_ap -> csrc/pair_tn.h)
        kernel, flops, split = "pair_tn_kernel<2, 2, 2, 0, 0, 2>", 2.0 * 4 * H * H * T * B, 3
    elif family == "lstm_wgrad_hh":
        kernel, flops = _cname("cpg_gemm_tn_kernel_name", T * B, 4 * H, H, 0), 2.0 * 4 * H * H * T * B
        split = 2 if kernel.endswith(", 1>") else 1
    else:
        return None
    ach = flops / (avg_us * 1e-6) / 1e12 if avg_us > 0 else 0.0
    peak = {0: PEAK_F32_MFMA_TFLOPS, 1: PEAK_SPLIT_TFLOPS, 2: PEAK_BF16_MFMA_TFLOPS, 3: PEAK_PAIR_TFLOPS}[int(split)]
    bf16_gates = bool(bf16 and family in ("fwd_persist", "fwd_step", "bwd_step") and L.cpg_gru_gates_bf16(B, H, 0) == 1)
    nbytes = family_bytes(family, dims, bf16_gates)
    gbs = nbytes / (avg_us * 1e-6) / 1e9 if (nbytes and avg_us > 0) else 0.0
    mfma_frac, hbm_frac = ach / peak, gbs / HBM_PEAK_GBS
    grid = None
    if family == "bwd_step" and kernel.startswith("gru_step_bwd_dl_kernel<"):   # <BM, BN, stages, engine, wave rows, wave columns>
        ta = [int(x) for x in kernel[kernel.index("<") + 1:-1].split(",")]
        if len(ta) == 6:
            grid = (B // ta[0]) * (H // ta[1]) * nd * 64 * ta[4] * ta[5]
    traffic = pmc_traffic(kernel, grid)
    pipe = {1: "bf16 MFMA x6 on 3-way split operands (f32-grade): 2500/6", 0: "exact f32 MFMA: 157.3", 2: "bf16 MFMA: 2500",
            3: "f16 MFMA x3 on f16-pair operands (f32-grade): 2500/3"}[int(split)]
    r = {"kernel": kernel, "avg_launch_us": round(avg_us, 2), "launches_timed": launches, "traffic": traffic,
         "mfma": {"achieved": round(ach, 2), "peak": round(peak, 1), "unit": "TFLOP/s", "frac": round(mfma_frac, 4), "pipe": pipe,
                  "flops_per_launch": flops, "frac_of_f32_mfma_peak": round(ach / PEAK_F32_MFMA_TFLOPS, 4)},
         "hbm": {"achieved": round(gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(hbm_frac, 4),
                 "algorithmic_bytes_per_launch": nbytes,
                 "counter_frac": (round(traffic / (avg_us * 1e-6) / 1e9 / HBM_PEAK_GBS, 4) if (traffic and avg_us > 0) else None)}}
    if hbm_frac > mfma_frac:
        r.update(bound="hbm", achieved=round(gbs, 1), peak=HBM_PEAK_GBS, unit="GB/s", frac=round(hbm_frac, 4))
    else:
        r.update(bound="mfma", achieved=round(ach, 2), peak=round(peak, 1), unit="TFLOP/s", frac=round(mfma_frac, 4))
    return r


def model_kwargs(z_dim, enc_h, enc_layers=1, emb_dim=150, cell='gru', dec_layers=1):
    return dict(
        z_dim=z_dim, c_dim=2, emb_dim=emb_dim, pretrained_emb=None, freeze_embeddings=False, flow=0, flow_type='',
        E_args=dict(h_dim=enc_h, biGRU=True, layers=enc_layers, p_dropout=0.0, cell=cell),
        G_args=dict(G_class='gru', GRU_args=dict(p_word_dropout=0.3, p_out_dropout=0.3, skip_connetions=False, cell=cell, layers=dec_layers),
                    deconv_args=dict()),
        C_args=dict(min_filter_width=3, max_filter_width=5, num_filters=100, dropout=0.5))


def train_flops_per_seq(T, E, He, Z, V, R, B, gates=3):
    """Executed FLOPs (2*MAC) of one training step per sequence on this implementation (token-table form), for the
    whole-step rate quoted in `extra`; the algorithmic count with the dense W_ih product is SURVEY 8d's."""
    Hd = Z + 2
    rec = 2 * T * 2 * gates * He * He + T * 2 * gates * Hd * Hd    # recurrent products, fwd
    small = 2 * gates * Hd * Hd + 2 * 2 * 2 * He * Z + T * 2 * Hd * V + 2 * 2 * Z * R
    fwd = rec + small
    return fwd + 2 * rec + 2 * small + 3 * 2 * B * Z                  # bwd: dh product + dW product (+ Gram MMD)


def host_cpu():
    """(model string, physical cores, logical cores) of the box's host CPU - every CPU baseline states the PHYSICAL cores it used."""
    model = "unknown"
    try:
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("model name"):
                model = ln.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    logical = os.cpu_count() or 1
    try:
        import psutil
        phys = psutil.cpu_count(logical=False) or logical
    except Exception:
        phys = logical
    return model, int(phys), int(logical)


def _cpu_case(tag, B, He, Z, full, nsteps, T, V, budget_s, min_steps=4):
    """One SURVEY 8(d) case: median step time of the torch-CPU restatement after 3 warm-up steps, at most `nsteps` timed steps, stopped
    early only when `budget_s` of host time is exhausted (the record says how many steps ran)."""
    from oracle import torch_ref
    from cpg.synth import synth_ids
    torch.manual_seed(1238)
    m = torch_ref.RefWAE(V, 150, He, 1, Z)
    tr = torch_ref.Trainer(m)
    rnd = dict(rf_w=torch.randn(Z, 500), rf_b=2 * np.pi * torch.rand(500))
    ids = synth_ids(B, T, V, torch.Generator().manual_seed(1))
    ts = []
    note("  cpu case: " + tag)
    t_case = time.perf_counter()
    for i in range(nsteps + 3):
        t0 = time.perf_counter()
        tr.step(ids, rnd, full_mmd=full)
        ts.append(time.perf_counter() - t0)
        if time.perf_counter() - t_case > budget_s and len(ts) >= min_steps:   # bounded sample
            break
    warm = min(3, len(ts) - 1)
    dt = float(np.median(ts[warm:]))
    return {"case": tag, "seq_per_s": round(B / dt, 1), "s_per_step": round(dt, 4), "steps": len(ts) - warm, "warmup": warm}


def _cpu_case_guarded(q, args):
    try:
        torch.set_num_threads(args[-1])
        q.put(_cpu_case(*args[:-1]))
    except MemoryError as e:
        q.put({"case": args[0], "failed": "MemoryError: " + str(e)[:120]})
    except RuntimeError as e:       # ATen's allocator raises RuntimeError("... not enough memory ...")
        q.put({"case": args[0], "failed": "RuntimeError: " + str(e)[:160]})


def cpu_baseline(T, V, threads, budget_s=70.0):
    """The torch-CPU restatement of the reference's training step (oracle/torch_ref.py: nn.GRU / F.cross_entropy / autograd /
    Adam exactly as train_vae.py drives them, pinned to the golden vectors in tests/test_oracle_golden.py) timed on the
    host cores at SURVEY 8(d)'s cases: (i) config A / batch 32, (ii) config A / batch 2048, (iii) config B / batch 2048 - the batch-2048
    cases BOTH with the reference-faithful [N,N,D] full-kernel MMD (/root/reference/losses.py:47-56,96-108: 91 % of the reference's step
    there) and with it disabled.  `value` is config B with the term off (this bench's dimensions; the comparable arithmetic).  Median of
    20 steps after 3 warm-up; the [N,N,D] cases are bounded samples (a step takes seconds to minutes: the record says how many steps ran),
    and the z = 510 one runs in a child process under a wall-clock limit - it needs 3 x 8.6 GB of kernel inputs plus autograd's copies -
    reported as not finished / out of memory if so."""
    torch.set_num_threads(threads)
    cases = []
    for tag, B, He, Z, full, nsteps, bud in (
            ("config B (enc h=512, z=510), batch 2048, full-kernel MMD off", 2048, 512, 510, False, 20, budget_s),
            ("config A (reference defaults: enc h=80, z=100), batch 32, all four regularisers", 32, 80, 100, True, 20, budget_s / 4),
            ("config A, batch 2048, full-kernel MMD off", 2048, 80, 100, False, 20, budget_s / 2),
            ("config A, batch 2048, WITH the [N,N,D] full-kernel MMD (all four regularisers, as the reference runs)", 2048, 80, 100, True, 5, budget_s / 3)):
        cases.append(_cpu_case(tag, B, He, Z, full, nsteps, T, V, bud, min_steps=4 if not (full and B > 32) else 2))
    # config B with the [N,N,D] form: child process, wall-clock limit (it may not fit / finish)
    import multiprocessing as mp
    tag = "config B, batch 2048, WITH the [N,N,D] full-kernel MMD"
    limit = max(30.0, budget_s)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    pr = ctx.Process(target=_cpu_case_guarded, args=(q, (tag, 2048, 512, 510, True, 2, T, V, limit * 0.6, 2, threads)))
    note("  cpu case (child process, %.0f s limit): %s" % (limit, tag))
    res = None
    try:
        pr.start()
        pr.join(limit)
        if pr.is_alive():
            pr.terminate()
            pr.join(5)
            res = {"case": tag, "failed": "not finished within %.0f s of wall clock (3 x 8.6 GB kernel inputs + autograd copies; one step takes longer than the bound)" % limit}
        elif not q.empty():
            res = q.get_nowait()
        else:
            res = {"case": tag, "failed": "child exited with code %s (killed by the kernel's OOM handling if -9)" % pr.exitcode}
    except Exception as e:       # no spawn in this environment: say so
        res = {"case": tag, "failed": "could not run: " + str(e)[:120]}
    cases.append(res)
    return cases


XGMI_LINK_GBS = 153.0   # one xGMI link, per direction (MI355X_MICROARCH.md); 7 links per GPU


def predicted_scaling(step_ms, grad_bytes, world, overlap_frac=0.58):
    """DESIGN.md 7's model of the weak-scaling efficiency at N ranks: the step of one rank + the part of the gradient all-reduce that
    does not hide under the encoder BPTT (buckets covering `overlap_frac` of the buffer are reduced while it runs; the rest - embedding +
    encoder recurrence - after the backward pass), ring all-reduce over all peer links."""
    if world <= 1:
        return 1.0
    ring_ms = 2.0 * (world - 1) / world * grad_bytes / (XGMI_LINK_GBS * min(world - 1, 7)) / 1e9 * 1e3
    exposed = (1.0 - overlap_frac) * ring_ms + 0.03   # + ~30 us of launch / synchronisation per collective
    return round(step_ms / (step_ms + exposed), 4)


def note(msg):
    """progress on stderr (stdout carries the one JSON line)"""
    print(f"[bench {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def _free_port():
    import socket
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    p = sk.getsockname()[1]
    sk.close()
    return p


def spawn_command(gpus, argv, port):
    """The launch line the driver uses for N > 1 (one rank per GPU over RCCL), built here when bench.py is started WITHOUT it."""
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={gpus}", "--master-addr", "127.0.0.1",
            "--master-port", str(port), os.path.abspath(__file__), *argv]


def maybe_self_spawn(args):
    """`python bench.py --gpus N` with no WORLD_SIZE in the environment re-executes itself as N ranks through
    torch.distributed.run (same arguments).  With fewer visible GPUs than ranks (a 1-GPU box) the ranks share devices:
    RCCL refuses two ranks on one device, so the collectives run on gloo and the line says so - a functional run of the
    N > 1 code path, not a scaling measurement."""
    if args.gpus <= 1 or "WORLD_SIZE" in os.environ:
        return
    import subprocess
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    ngpu = torch.cuda.device_count() if torch.cuda.is_available() else 0
    if args.dist_selftest or ngpu < args.gpus:
        env["CPG_DIST_BACKEND"] = "gloo"
    if 0 < ngpu < args.gpus:
        env["CPG_SHARED_DEVICE"] = "1"   # persistent kernels need every CU of the device to themselves: cpg.ops switches them off
    cmd = spawn_command(args.gpus, sys.argv[1:], _free_port())
    note("self-spawn: " + " ".join(cmd[1:8]) + " ...")
    sys.exit(subprocess.call(cmd, env=env))


def launch_count_per_step(step_fn):
    """Kernel launches of ONE training step (torch.profiler device-activity records; None when the profiler is unavailable or
    switched off with CPG_BENCH_NO_TORCH_PROFILER=1, e.g. under rocprofv3)."""
    if os.environ.get("CPG_BENCH_NO_TORCH_PROFILER"):
        return None
    try:
        from torch.profiler import profile, ProfilerActivity
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            step_fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and not e.name.lower().startswith(("memcpy", "memset")))
        return n or None
    except Exception as e:   # noqa: BLE001 - a diagnostic count must never fail the bench
        note(f"launch count unavailable: {e!r}")
        return None


_PROBE_HUNG = []   # set when the collectives probe left a thread stuck inside RCCL: main() then leaves through os._exit


def rccl_probe(dev, grad_numel, backend, world, iters=20):
    """Times the two collectives of the path on their real payloads: the SUM all-reduce of a flat f32 gradient buffer of the
    model's size, and the all-gather of one CLaSS round's rows (cpg.dist.allgather_rows on a [65536/world, 26] int16 + f32
    frame).  HIP events on the current stream; RCCL enqueues on its own stream and the process group makes the current
    stream wait for it (work.wait()), so the events bracket the collective."""
    import torch.distributed as tdist
    from cpg import dist as cdist
    on_gpu = backend == "nccl"
    buf = torch.zeros(grad_numel, device=dev if on_gpu else "cpu", dtype=torch.float32)
    rows = torch.zeros(65536 // world, 26 + 100, device=dev if on_gpu else "cpu", dtype=torch.float32)

    def timed(fn):
        for _ in range(3):
            fn()
        if on_gpu:
            torch.cuda.synchronize()
        tdist.barrier()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        if on_gpu:
            torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters * 1e3
    ar = timed(lambda: tdist.all_reduce(buf))
    ag = timed(lambda: cdist.allgather_rows(rows))
    nbytes = grad_numel * 4
    # self-diagnosis of a first real multi-GPU run (round-4 verdict #10): the ranks the RCCL communicator ITSELF reports (the library's
    # own communicator, ncclCommCount) next to the launcher's WORLD_SIZE, and the all-reduce against the xGMI model of DESIGN.md 7 -
    # a ring moves 2 (N-1)/N of the payload over every GPU's links; one link = 153 GB/s, a GPU has 7 (one per peer at N = 8)
    ranks_seen = None
    if on_gpu and not os.environ.get("CPG_SHARED_DEVICE"):
        # The probe builds a SECOND communicator (ncclCommInitRank on every rank).  It must not take the bench line down: (i) the ranks
        # first agree (MIN all-reduce) that every one of them can reach the library's entry points - a rank that cannot would leave
        # the others waiting inside the init; (ii) the init runs on a watchdog thread - after 45 s the run goes on without the number
        # and leaves through os._exit at the end (a thread stuck inside RCCL cannot be joined).
        import threading
        ok = torch.ones(1, device=dev)
        api = None
        try:
            api = cdist._CApi()
            if not hasattr(api, "count"):
                raise RuntimeError("cpg_comm_count missing")
        except Exception:
            ok.zero_()
        tdist.all_reduce(ok, op=tdist.ReduceOp.MIN)
        if float(ok.item()) < 1.0:
            ranks_seen = "unavailable: a rank cannot reach the library's RCCL entry points"
        else:
            res = {}

            def work():
                try:
                    lc = cdist.LibComm(tdist.get_rank(), world, api=api)
                    res["n"] = lc.ranks_seen()
                    lc.close()
                except Exception as exc:
                    res["err"] = "unavailable: %s" % (str(exc)[:80],)
            th = threading.Thread(target=work, daemon=True)
            th.start()
            th.join(45.0)
            if th.is_alive():
                ranks_seen = "timeout: the library communicator's init did not return within 45 s"
                _PROBE_HUNG.append(True)
            else:
                ranks_seen = res.get("n", res.get("err"))
    ring = 2.0 * (world - 1) / world * nbytes
    t_one, t_all = ring / XGMI_LINK_GBS / 1e9 * 1e3, ring / (XGMI_LINK_GBS * min(world - 1, 7)) / 1e9 * 1e3
    return {"backend": backend, "ranks": world, "ranks_seen": ranks_seen, "allreduce_ms": round(ar, 4), "allreduce_bytes": nbytes,
            "allreduce_busbw_GBs": round(2.0 * (world - 1) / world * nbytes / (ar * 1e-3) / 1e9, 2),
            "allreduce_model_ms": {"one_link_153GBs": round(t_one, 4), "all_peer_links": round(t_all, 4),
                                   "measured_over_all_links_model": round(ar / t_all, 2) if t_all > 0 else None},
            "allgather_ms": round(ag, 4), "allgather_rows_per_rank": rows.shape[0], "allgather_row_bytes": rows.shape[1] * 4,
            "shared_device": bool(os.environ.get("CPG_SHARED_DEVICE")),
            "overlap": "gradient buckets (decoder, encoder heads) are all-reduced while the encoder BPTT still runs (cpg.optim)"}


def dist_selftest(args):
    """CPU-only check of the N > 1 launcher and the collectives plumbing (tests/test_dist_gloo.py runs it with 2 ranks):
    no GPU work at all, prints one JSON line with the `rccl` object measured over gloo."""
    import torch.distributed as tdist
    from cpg import dist as cdist
    world, rank, local = cdist.init(backend="gloo")
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    probe = rccl_probe(None, 1 << 16, "gloo", world, iters=3) if world > 1 else None
    if world > 1:
        tdist.barrier()
    if rank == 0:
        print(json.dumps({"selftest": "dist", "n_gpus": world, "rccl": probe}))


DUMP_LIMIT_BYTES = 64 << 20   # --dump-outputs: at most this much in all


def dump_outputs(outdir, out, model):
    """--dump-outputs: what the timed step handed its caller (train_step's dict) and the parameters it left behind, as
    <outdir>/<name>.npy (float32; python scalars float64).  Over DUMP_LIMIT_BYTES in all, each array above its share keeps a
    fixed, seeded sample of its flattened elements (<name>.sample.npy; the same indices on every run)."""
    arrays = {}
    for k, v in out.items():
        if torch.is_tensor(v):
            arrays[k] = v.detach().float().cpu().numpy()
        elif isinstance(v, (int, float)):
            arrays[k] = np.asarray(v, dtype=np.float64)
    for k, v in model.named_parameters():
        arrays["param." + k] = v.detach().float().cpu().numpy()
    os.makedirs(outdir, exist_ok=True)
    budget = DUMP_LIMIT_BYTES - (1 << 20)      # (room for the .npy headers)
    share = budget // max(len(arrays), 1)
    for k, a in sorted(arrays.items()):
        name = k
        if sum(b.nbytes for b in arrays.values()) > budget and a.nbytes > share:
            idx = np.sort(np.random.default_rng(1238).choice(a.size, share // a.itemsize, replace=False))
            a, name = a.reshape(-1)[idx], k + ".sample"
        np.save(os.path.join(outdir, name + ".npy"), a)


def train_leg(args, dev, rank, world, dtype, hidden, enc_layers, batch, seq_len, steps, warmup, min_sustain_s=0.0, graph=False, z_dim=None,
              cell=None, dec_layers=1, opts=None, dump_dir=None):
    """One timed WAE-training leg: builds the model at the given dimensions, W untimed steps, EXACTLY `steps` timed steps
    bracketed by barrier + synchronize, max over ranks.  Returns the numbers of the leg (rank 0 builds the roofline rows).
    min_sustain_s > 0: afterwards the same step keeps running until that much wall time has passed (`sustained`): the timed
    region of the default K=20 is 0.14 s, too short for an SMI sampler to see the GPU busy.
    dump_dir: rank 0 writes the last timed step's outputs there (dump_outputs) before anything else runs a step."""
    import cfg
    import losses
    from cpg import dist as cdist
    from cpg import ops
    from cpg.synth import synth_ids
    from models.model import RNN_VAE
    import train_vae as tv

    cell = cell or args.cell
    ops.set_compute_mode(dtype)
    for k, v in (opts or {}).items():      # launch-policy options of this leg (cpg_set_option; KNOBS.md), returned to the policy below
        ops.set_option(k, v)
    T, V, B, Hh = seq_len, 24, batch, hidden
    Z, E, R = (Hh - 2 if z_dim is None else z_dim), 150, 500
    torch.manual_seed(1238)
    model = RNN_VAE(n_vocab=V, max_seq_len=T, **model_kwargs(Z, Hh, enc_layers=enc_layers, cell=cell, dec_layers=dec_layers)).to(dev)
    model.device = dev
    losses.rf.clear()
    losses._rf_basis(torch.zeros(1, Z, device=dev), R, False)          # same basis on every rank (same seed)
    model.use_device_rng(1238 + 7919 * rank)                            # rank-distinct draws
    losses.set_prior_sampler(lambda z: model._randn(z.shape[0], z.shape[1]))
    cdist.broadcast_params(model.parameters())
    reduce_fn = cdist.allreduce_sum if world > 1 else None
    losses.set_distributed(reduce_fn, world, gather_fn=cdist.allgather_equal, rank=rank)
    cfgv = cfg.Bunch(lr=1e-3, clip_grad=5.0, z_regu_loss='mmdrf', lambda_logvar_L1=0.0, lambda_logvar_KL=1e-3,
                     beta=cfg.Bunch(start=cfg.Bunch(val=1.0, iter=0), end=cfg.Bunch(val=2.0, iter=40000)))
    trainer = tv.make_optimizer(cfgv, model, reduce_fn, world)
    g = torch.Generator().manual_seed(1238 + rank)
    pool = [synth_ids(B, T, V, g).to(dev) for _ in range(8)]

    graphed = tv.GraphedTrainStep(cfgv, model, trainer) if graph else None   # first calls eager, then capture, then replays

    def step(it):
        if graphed is not None:
            return graphed(pool[it % len(pool)], it)
        return tv.train_step(cfgv, model, trainer, pool[it % len(pool)], it)

    for it in range(max(warmup, 5) if graph else warmup):
        step(it)
    torch.cuda.synchronize()
    cdist.barrier()
    torch.cuda.synchronize()
    ops.PROFILE = []
    t0 = time.perf_counter()
    for it in range(steps):
        out = step(warmup + it)
    t_enqueued = time.perf_counter() - t0   # host time to enqueue the K steps (no host sync inside a step)
    torch.cuda.synchronize()
    cdist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    prof, ops.PROFILE = ops.PROFILE, None
    tmax = torch.tensor([dt], device=dev, dtype=torch.float64)
    per_rank = None
    if world > 1:
        # every rank's own time for the K steps (a straggler - a throttled GPU, a slow xGMI link - shows here), then the max
        mine = torch.zeros(world, device=dev, dtype=torch.float64)
        mine[rank] = dt
        cdist.allreduce_sum(mine)
        per_rank = [round(float(x) / steps * 1e3, 3) for x in mine.tolist()]
        cdist.allreduce_max(tmax)
    dt = float(tmax.item())
    loss_val = float(out["L_vae"].item())
    assert np.isfinite(loss_val), "non-finite loss in the timed region"
    if dump_dir and rank == 0:
        dump_outputs(dump_dir, out, model)
    ops.check_persistent()
    ms = dt / steps * 1e3
    res = {"value": round(B * world * steps / dt, 1), "ms_per_step": round(ms, 3), "steps": steps, "warmup": warmup,
           "loss_last_step": round(loss_val, 4), "host_enqueue_ms_per_step": round(t_enqueued / steps * 1e3, 3),
           "grad_numel": trainer.flat_g.numel(), "ms_per_step_per_rank": per_rank,
           "launches_per_step": None if graph else launch_count_per_step(lambda: step(warmup + steps))}
    if min_sustain_s > 0:
        # same step, same model, until min_sustain_s of wall time: per-step time over ALL of these iterations
        it, n = warmup + steps + 1, 0
        torch.cuda.synchronize()
        cdist.barrier()
        ts = time.perf_counter()
        chunk = max(steps, 10)
        while True:
            for _ in range(chunk):
                step(it)
                it += 1
            n += chunk
            torch.cuda.synchronize()
            go = torch.tensor([1.0 if time.perf_counter() - ts < min_sustain_s else 0.0], device=dev)
            if world > 1:
                cdist.allreduce_max(go)          # every rank runs the same number of chunks
            if go.item() == 0.0:
                break
        cdist.barrier()
        ds = time.perf_counter() - ts
        res["sustained"] = {"steps": n, "wall_s": round(ds, 3), "ms_per_step": round(ds / n * 1e3, 3),
                            "value": round(B * world * n / ds, 1)}
        ops.check_persistent()
    if rank == 0:
        # kernel families of the step, timed with HIP events on their launch streams inside the timed region (cpg.ops._prof);
        # the roofline object carries the family with the largest share of the step, the others follow in `extra`
        fams = {}
        for fam, e0, e1, launches, dims in prof:
            # a launch deferred to the side stream (the decoder's dW_hh under the chain of small launches) is its own row: its duration
            # is stretched by what it runs beside and says nothing about the kernel's rate - the main-stream launches of the same
            # kernel do (round-4 verdict: the family average mixed the two)
            key = (fam, dims["B"], dims["H"], dims["ndir"], dims["T"], bool(dims.get("side")))
            f = fams.setdefault(key, {"ms": 0.0, "launches": 0, "dims": dims, "family": fam})
            f["ms"] += e0.elapsed_time(e1)
            f["launches"] += launches
        rows = []
        for f in fams.values():
            avg_us = f["ms"] * 1e3 / max(f["launches"], 1)
            r = family_roofline(f["family"], f["dims"], avg_us, f["launches"])
            if r is None:
                continue
            r["family"] = f["family"] + ("_pair" if f["dims"]["ndir"] == 2 else "") + ("_side" if f["dims"].get("side") else "")
            if f["dims"].get("side"):
                r["note"] = "side stream, overlapped with the main stream's launches: not a kernel rate"
            r["ms_per_step"] = round(f["ms"] / steps, 3)
            r["share_of_step"] = round(f["ms"] / steps / ms, 4)
            rows.append(r)
        rows.sort(key=lambda r: -r["ms_per_step"])
        by_kernel = {}
        for r in rows:   # single-direction and paired launches of one kernel: rank kernels by their summed share
            by_kernel[r["kernel"]] = by_kernel.get(r["kernel"], 0.0) + r["ms_per_step"]
        top_kernel = max(by_kernel, key=by_kernel.get) if by_kernel else None
        roofline = next((r for r in rows if r["kernel"] == top_kernel and "note" not in r),
                        {"bound": "mfma", "kernel": None, "achieved": 0.0, "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s",
                         "frac": 0.0, "traffic": None})
        roofline = dict(roofline)
        roofline["kernel_ms_per_step_all_launch_shapes"] = round(by_kernel.get(top_kernel, 0.0), 3)
        gates = 3 if cell == "gru" else 4
        step_tflops = train_flops_per_seq(T, E, Hh, Z, V, R, B, gates) * B / (ms * 1e-3) / 1e12
        res.update(roofline=roofline, kernel_families=[r for r in rows if r["kernel"] != top_kernel or r["family"] != roofline.get("family")],
                   executed_step_tflops_per_gpu=round(step_tflops, 2),
                   executed_step_frac_of_f32_peak=round(step_tflops / PEAK_F32_MFMA_TFLOPS, 4))
    del trainer, model, pool
    losses.set_distributed(None, 1)
    ops.set_compute_mode('f32')
    for k in (opts or {}):
        ops.set_option(k, None)
    if os.environ.get("CPG_BENCH_EMPTY_CACHE"):
        torch.cuda.empty_cache()   # (default: keep the caching allocator's blocks for the next leg - 288 GB of HBM hold every leg)
    return res


def workload_text(args, dtype, Hh, enc_layers, B, T, cell=None, dec_layers=1):
    cell = cell or args.cell
    Z = Hh - 2
    cfg_tag = ("BASELINE.json configs[1]" if (Hh, T, enc_layers, B, dec_layers) == (512, 25, 1, 2048, 1)
               else (f"BASELINE.json configs[4] dimensions, {cell.upper()} cells, "
                     + ("1-layer decoder as in the reference" if dec_layers == 1 else
                        f"{dec_layers}-layer decoder AS NAMED by configs[4] (extension: the reference hard-wires one layer - parity unpinned vs the reference)"))
               if (Hh, T, enc_layers) == (1024, 50, 2) else "non-default dimensions")
    C = cell.upper()
    return (f"WAE train step ({cfg_tag}): bi{C} encoder h={Hh} x{enc_layers}, z={Z}, {C} decoder h={Hh} x{dec_layers}, emb 150, vocab 24, "
            f"batch {B}/GPU, T={T}; "
            + ("GRU = the reference's only cell (parity pinned)" if cell == "gru" else
               "LSTM = extension named by BASELINE.json (torch.nn.LSTM semantics; parity unpinned vs the GRU-only reference)")
            + ("; f32 storage, f32-grade products on f16-pair MFMA (22-bit significands, f32 accumulate)" if dtype == "f32" else
               "; bf16 mode: bf16-rounded recurrent operands, f32 accumulate / state / master weights, bf16 saved gates (not the parity path)"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=2048, help="sequences per GPU per step")
    ap.add_argument("--hidden", type=int, default=512, help="encoder h_dim and decoder hidden (z_dim = hidden-2)")
    ap.add_argument("--seq-len", type=int, default=25)
    ap.add_argument("--enc-layers", type=int, default=1, help="encoder biGRU layers (BASELINE.json configs[4] uses 2; the decoder stays 1 layer as in the reference)")
    ap.add_argument("--dec-layers", type=int, default=1, help="decoder RNN layers (1 = the reference; 2 = BASELINE.json configs[4]'s \"2-layer dec\", an extension)")
    ap.add_argument("--cell", default="gru", choices=["gru", "lstm"], help="gru = the reference's cell (parity pinned); lstm = extension")
    ap.add_argument("--dtype", default="f32", choices=["f32", "bf16"],
                    help="f32 = f32-grade products (the parity path, the headline line); bf16 = bf16 recurrent products "
                         "(cfg.hw.dtype='bf16': one bf16 MFMA per block, f32 accumulate / master weights)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-class", action="store_true")
    ap.add_argument("--no-extra-legs", action="store_true", help="skip extra.bf16_mode / extra.config_c / the sustained region")
    ap.add_argument("--sustain-s", type=float, default=2.5, help="wall seconds of the sustained region after the K timed steps")
    ap.add_argument("--cpu-budget-s", type=float, default=70.0, help="host seconds for the config-B cpu_baseline case (20 steps of ~2.4 s fit); the other cases take fractions of it")
    ap.add_argument("--class-proposals", type=int, default=1000000, help="z proposals of the CLaSS leg (BASELINE.json configs[3]: 1 M in total, sharded over the ranks)")
    ap.add_argument("--all-legs", action="store_true", help="N > 1: also run the config-C leg (skipped by default to bound the wall time)")
    ap.add_argument("--dist-selftest", action="store_true", help="CPU-only check of the N>1 launcher + collectives (gloo); no GPU work")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the headline leg's last timed step (train_step's outputs, the updated parameters) to DIR/<name>.npy")
    args = ap.parse_args()

    maybe_self_spawn(args)
    if args.dist_selftest:
        return dist_selftest(args)

    # launched by an outside torch.distributed.run with more ranks on this node than it has GPUs (a 1-GPU box): the same functional fallback
    # as the self-spawn above - RCCL refuses two ranks on one device ("Duplicate GPU detected"), so gloo carries the collectives and the
    # persistent kernels (which need every CU of a device to themselves) are switched off.  Decided BEFORE cpg.ops is imported.
    if "WORLD_SIZE" in os.environ and torch.cuda.is_available():
        lw = int(os.environ.get("LOCAL_WORLD_SIZE", os.environ["WORLD_SIZE"]))
        if 0 < torch.cuda.device_count() < lw:
            os.environ.setdefault("CPG_DIST_BACKEND", "gloo")
            os.environ["CPG_SHARED_DEVICE"] = "1"
            os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    from cpg import dist as cdist
    world, rank, local = cdist.init()
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    assert torch.cuda.is_available(), "bench.py needs MI355X GPUs; there is no CPU path"
    local = cdist.local_device(local)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    backend = torch.distributed.get_backend() if world > 1 else None

    T, B, Hh = args.seq_len, args.batch, args.hidden
    t_start = time.perf_counter()
    note("headline leg")
    head = train_leg(args, dev, rank, world, args.dtype, Hh, args.enc_layers, B, T, args.steps, args.warmup,
                     0.0 if args.no_extra_legs else args.sustain_s, dec_layers=args.dec_layers, dump_dir=args.dump_outputs)
    extra, full = {}, {}
    default_shape = (Hh, T, args.enc_layers, B, args.dtype, args.cell, args.dec_layers) == (512, 25, 1, 2048, "f32", "gru", 1)

    def leg(key, what, r, brief=False, **more):
        """One extra leg: the compact form goes into the JSON line, the full record (every family's two roofs) to bench_full.json."""
        if rank != 0:
            return
        full[key] = dict(workload=what, **{k: r[k] for k in ("value", "ms_per_step", "steps", "warmup", "roofline", "kernel_families",
                                                             "launches_per_step", "host_enqueue_ms_per_step") if k in r}, **more)
        extra[key] = dict(workload=what, value=r["value"], unit="seq/s", ms_per_step=r["ms_per_step"], steps=r["steps"],
                          roofline=compact_roofline(r.get("roofline")), **more)
        if brief:    # (the line stays under 10 KB: the families of this leg are in bench_full.json only)
            extra[key]["workload"] = what.split(":")[0]   # the dimensions follow in bench_full.json
            extra[key]["roofline"] = {k: v for k, v in extra[key]["roofline"].items() if k in ("bound", "kernel", "frac", "avg_launch_us")}
        else:
            extra[key]["workload"] = what.split("; ")[0]   # dimensions only: the explanatory tail is in bench_full.json
            extra[key]["families"] = compact_families(r.get("kernel_families"))

    if default_shape and not args.no_extra_legs:
        if world == 1:
            # what exactness costs: the same step with every recurrent product on IEEE-f32-exact pipes (backward step + dW_hh on the
            # exact-f32 MFMA, persistent forward on the bf16 triple whose six-term sum is exact to 2^-26) - round-4 verdict: `dtype: f32`
            # alone hid that the headline's products are 22-bit f16 pairs
            note("exact-f32 leg")
            leg("exact_f32", workload_text(args, "f32", Hh, args.enc_layers, B, T).replace(
                    "f32-grade products on f16-pair MFMA (22-bit significands, f32 accumulate)",
                    "EXACT-f32 recurrent products (options gru_bwd_engine=exact, f32_engine=bf16x3): v_mfma_f32_16x16x4_f32 + bf16x3 six-term split"),
                train_leg(args, dev, rank, world, "f32", Hh, args.enc_layers, B, T, args.steps, args.warmup,
                          opts=dict(gru_bwd_engine="exact", f32_engine="bf16x3")), brief=True)
        note("bf16-mode leg")
        leg("bf16_mode", workload_text(args, "bf16", Hh, args.enc_layers, B, T),
            train_leg(args, dev, rank, world, "bf16", Hh, args.enc_layers, B, T, args.steps, args.warmup))
        # BASELINE.json configs[1] AS NAMED: "hidden=512 1-layer LSTM, batch=2048, seq_len<=25, bf16" - the LSTM extension, both modes
        note("LSTM legs (configs[1] as named)")
        leg("lstm", workload_text(args, "f32", Hh, args.enc_layers, B, T, "lstm"),
            train_leg(args, dev, rank, world, "f32", Hh, args.enc_layers, B, T, args.steps, args.warmup, cell="lstm"))
        leg("lstm_bf16", workload_text(args, "bf16", Hh, args.enc_layers, B, T, "lstm"),
            train_leg(args, dev, rank, world, "bf16", Hh, args.enc_layers, B, T, args.steps, args.warmup, cell="lstm"))
        if world == 1 or args.all_legs:   # a multi-GPU run is about the scaling of the headline step: keep its wall time bounded
            if world == 1:
                note("graph-replay legs")
                r = train_leg(args, dev, rank, world, "f32", Hh, args.enc_layers, B, T, args.steps, args.warmup, graph=True)
                extra["graph_replay"] = {"what": "the same step replayed from ONE captured hipGraph (cfg.hw.graph)", "value": r["value"],
                                         "ms_per_step": r["ms_per_step"], "host_enqueue_ms_per_step": r["host_enqueue_ms_per_step"]}
                # the reference's own defaults (config A: enc h=80, z=100, decoder h=102) at its default batch of 32: host-bound eagerly
                ra = {}
                for tag, gflag in (("eager", False), ("graph", True)):
                    rr = train_leg(args, dev, rank, world, "f32", 80, 1, 32, 25, 200, 20, graph=gflag, z_dim=100)
                    ra[tag] = {"value": rr["value"], "ms_per_step": rr["ms_per_step"], "host_enqueue_ms_per_step": rr["host_enqueue_ms_per_step"]}
                extra["config_a_batch32"] = {"workload": "reference defaults (enc h=80, z=100, dec h=102), batch 32, T=25, 200 steps", **ra}
            note("config-C leg")
            cB, cK, cW = 1024, max(3, min(args.steps, 6)), 2
            leg("config_c", workload_text(args, "f32", 1024, 2, cB, 50),
                train_leg(args, dev, rank, world, "f32", 1024, 2, cB, 50, cK, cW))
            if world == 1:   # configs[4] names LSTM cells: the extension at the same dimensions (persistent forward at h = 1024 since round 4)
                leg("config_c_lstm", workload_text(args, "f32", 1024, 2, cB, 50, "lstm", dec_layers=2),
                    train_leg(args, dev, rank, world, "f32", 1024, 2, cB, 50, cK, cW, cell="lstm", dec_layers=2), brief=True)
    rccl = None
    if world > 1:
        note("collectives probe")
        rccl = rccl_probe(dev, head["grad_numel"], backend, world)
    cls = None
    if not args.no_class:
        note("CLaSS leg")
        cls = class_bench(dev, N=args.class_proposals, cpu=(world == 1 and not args.no_cpu_baseline), rank=rank, world=world)
    if rank != 0:
        cdist.barrier()
        return
    note(f"timed region: {head['ms_per_step']:.3f} ms/step")
    extra.update({k: head[k] for k in ("loss_last_step", "host_enqueue_ms_per_step", "executed_step_tflops_per_gpu",
                                       "executed_step_frac_of_f32_peak")})
    lp, lg = profiled_launches()
    extra["launches_per_step"] = {"rocprofv3_kernel_trace": lp, "of_which_torch_glue": lg,
                                  "torch_profiler_device_records": head["launches_per_step"]}
    if "sustained" in head:
        extra["sustained"] = head["sustained"]
    extra["families"] = compact_families(head["kernel_families"])
    full["headline"] = {k: head[k] for k in ("roofline", "kernel_families") if k in head}
    line = {
        "metric": "peptide-seq/s per WAE training step", "value": head["value"], "unit": "seq/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": head["ms_per_step"],
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32 storage / f16x2-pair MFMA" if args.dtype == "f32" else args.dtype, "data": "synthetic",
        "config": {"workload": workload_text(args, args.dtype, Hh, args.enc_layers, B, T, dec_layers=args.dec_layers),
                   "global_batch": B * world, "seq_len": T, "parallelism": f"dp{world}"},
        "roofline": compact_roofline(head["roofline"], keep_all=True), "extra": extra,
    }
    line["config"]["step_launch"] = "eager (one host enqueue per kernel)"
    g = extra.get("graph_replay")
    forced = os.environ.get("CPG_BENCH_FORCE_GRAPH_LINE", "") == "1"   # (exercises this branch on a healthy box)
    if world == 1 and g and (forced or (head["host_enqueue_ms_per_step"] >= 0.9 * head["ms_per_step"] and g["ms_per_step"] < 0.97 * head["ms_per_step"])):
        # a host-bound box (the enqueue of a step took as long as the step: seen on one box in eight of the pool, 5.8 ms of enqueue against
        # 5.1 ms of device work): the product's remedy is cfg.hw.graph - the SAME train_step captured once and replayed (bit-identical,
        # DESIGN 5.7), K steps timed by the same bracket.  The line then carries that leg and says so; the eager numbers stay beside it.
        extra["eager_step"] = {"value": head["value"], "ms_per_step": head["ms_per_step"], "host_enqueue_ms_per_step": head["host_enqueue_ms_per_step"]}
        line["value"], line["ms_per_step"] = g["value"], g["ms_per_step"]
        line["config"]["step_launch"] = ("hipGraph replay (cfg.hw.graph): this run's eager step was HOST-bound "
                                         f"({head['host_enqueue_ms_per_step']} ms of enqueue per {head['ms_per_step']} ms step, extra.eager_step); "
                                         "kernel families / roofline are the eager leg's HIP-event timings of the same kernels")
    if rccl is not None:
        rccl["ms_per_step_per_rank"] = head.get("ms_per_step_per_rank")
        line["rccl"] = rccl
    line["extra"]["predicted_weak_scaling_efficiency"] = {
        "model": "DESIGN.md 7: step + exposed ring all-reduce at 153 GB/s x peer links (the measured efficiency is the driver's)",
        **{f"n{n}": predicted_scaling(head["ms_per_step"], head["grad_numel"] * 4, n) for n in (2, 4, 8)}}
    if world == 1 and not args.no_cpu_baseline:
        # ATen's CPU GRU forks/joins its thread pool at every time step: on the box's 256 hardware threads the step got SLOWER
        # than on 8 (minutes per step); 32 threads is about the best these shapes get.  Stated in the output.
        model, phys, logical = host_cpu()
        threads = min(32, phys)
        note("cpu baseline (torch-CPU restatement)")
        cases = cpu_baseline(T, 24, threads, args.cpu_budget_s)
        c0 = cases[0]
        line["cpu_baseline"] = {"value": c0["seq_per_s"], "unit": "seq/s", "cores": threads, "kind": "port",
                                "cpu": f"{model}: {phys} physical / {logical} logical cores; {threads} threads (= physical cores used; ATen's CPU GRU "
                                       "forks / joins its pool at every time step - more threads are slower)",
                                "sample": f"oracle/torch_ref.py (torch-CPU restatement of train_vae.py's step, ATen CPU kernels); {c0['case']}: median of "
                                          f"{c0['steps']} steps after {c0['warmup']} warm-up ({c0['s_per_step']} s/step; SURVEY 8d: 20 after 3)",
                                "cases": [({"case": c["case"], "seq_per_s": c["seq_per_s"], "steps": c["steps"]} if "failed" not in c
                                           else {"case": c["case"], "failed": c["failed"]}) for c in cases]}
    if cls is not None:
        full["class"] = cls
        line["class"] = compact_class(cls)
    line["extra"]["wall_s"] = round(time.perf_counter() - t_start, 1)
    full["line"] = line
    try:   # the verbose record (every family with both roofs, every CLaSS variant): a file next to the line, and stderr
        outdir = os.environ.get("CPG_BENCH_OUT", os.path.join(ROOT, "gpurun_out"))
        os.makedirs(outdir, exist_ok=True)
        with open(os.path.join(outdir, "bench_full.json"), "w") as fh:
            json.dump(full, fh)
    except OSError:
        pass
    print(json.dumps(line, separators=(",", ":")), flush=True)
    cdist.barrier()


def compact_roofline(r, keep_all=False):
    """The roofline object as it goes into the ONE JSON line: the binding roof's numbers, the kernel, both fractions."""
    if not r:
        return None
    out = {k: r.get(k) for k in ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "avg_launch_us") if k in r}
    if "mfma" in r:
        out["mfma_frac"], out["hbm_frac"] = r["mfma"]["frac"], r["hbm"]["frac"]
        out["frac_of_f32_mfma_peak"] = r["mfma"]["frac_of_f32_mfma_peak"]
    if keep_all:
        for k in ("launches_timed", "family", "ms_per_step", "share_of_step", "kernel_ms_per_step_all_launch_shapes"):
            if k in r:
                out[k] = r[k]
        if "mfma" in r:
            out["pipe"], out["flops_per_launch"] = r["mfma"]["pipe"], r["mfma"]["flops_per_launch"]
            out["algorithmic_bytes_per_launch"] = r["hbm"]["algorithmic_bytes_per_launch"]
    return out


def compact_families(rows):
    return [{"family": r.get("family"), "kernel": r["kernel"], "us": r["avg_launch_us"], "ms_per_step": r.get("ms_per_step"),
             "bound": r["bound"], "frac": r["frac"], "mfma_frac": r["mfma"]["frac"], "hbm_frac": r["hbm"]["frac"]} for r in (rows or [])]


def compact_class(c):
    out = {k: c[k] for k in ("workload", "metric", "value", "unit", "n_gpus", "scaling", "decoder_evals_per_s") if k in c}
    rf = c.get("roofline") or {}
    out["roofline"] = {k: rf.get(k) for k in ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "avg_launch_us")}
    out["variants"] = {k: {kk: v[kk] for kk in ("wall_s", "accepted_per_s", "proposals_per_s", "decoder_evals_per_s", "decode_kernel_ms",
                                                 "accepted_unique", "decoded") if kk in v} for k, v in c.get("variants", {}).items()}
    for k, v in c.get("variants", {}).items():
        if v.get("roofline"):
            out["variants"][k]["frac"] = v["roofline"]["frac"]
    if c.get("config_b_width"):
        w = c["config_b_width"]
        out["config_b_width"] = {k: ({kk: v[kk] for kk in ("wall_s", "accepted_per_s", "decoder_evals_per_s", "decode_chain_ms")} | {"frac": v["roofline"]["frac"], "kernel": v["roofline"]["kernel"]}
                                     if isinstance(v, dict) else v) for k, v in w.items()}
    if "cpu_baseline" in c:
        cb = c["cpu_baseline"]
        out["cpu_baseline"] = {k: cb[k] for k in ("value", "unit", "cores", "kind", "z_per_s", "decoder_evals_per_s", "accept_rate") if k in cb}
        out["cpu_baseline"]["sample"] = ("SURVEY 8d: sklearn GaussianMixture.sample + LogisticRegression.predict_proba + accept of 1e6 z, "
                                         "oracle beam-5 of 1e4 z on `cores` processes (full text: bench_full.json)")
    return out


def class_setup(dev, Z=100, K=100, seed=1238, enc_h=80):
    """SURVEY 8(d) synthetic CLaSS problem at the reference's default dims: proposal = diagonal GMM (K=100, means N(0,0.8^2),
    variances e^-2), two logistic-regression heads w ~ N(0,1/Z), b = 0, targets {amp: 1, tox: 0}."""
    import types
    from cpg.synth import SyntheticPeptideLoader
    from density_modeling import mogQ
    from models.model import RNN_VAE
    torch.manual_seed(seed)
    m = RNN_VAE(n_vocab=24, max_seq_len=25, **model_kwargs(Z, enc_h)).to(dev)
    m.device = dev
    rs = np.random.RandomState(seed)
    Q = mogQ.from_params(np.ones(K) / K, rs.randn(K, Z) * 0.8, np.full((K, Z), np.exp(-2.0)), device=dev)
    clf = lambda: types.SimpleNamespace(coef_=rs.randn(1, Z) / np.sqrt(Z), intercept_=np.zeros(1), classes_=np.array([0.0, 1.0]))
    Q.init_attr_classifiers({'amp': clf(), 'tox': clf()}, clf_targets={'amp': 1, 'tox': 0})
    Q.rng = 'device'
    ds = SyntheticPeptideLoader(4, 25, dev, size=16)
    return m, Q, ds


_BEAM_JOB = {}   # weights of class_cpu_baseline's forked workers (inherited through fork: nothing is pickled but the row range)


def _beam_chunk(job):
    """Worker of class_cpu_baseline (forked: numpy only, BLAS limited to one thread per process)."""
    a, b = job
    P, z, c = _BEAM_JOB["P"], _BEAM_JOB["z"][a:b], _BEAM_JOB["c"][a:b]
    from threadpoolctl import threadpool_limits
    from oracle import decode as odec
    with threadpool_limits(limits=1):
        hyps, _ = odec.beam(P, z, c, 25, beam_size=5, n_best=3)
    return sum(len(h[0]) - 1 for h in hyps)


def class_cpu_baseline(m, Q, n_score=1000000, n_decode=10000):
    """SURVEY 8(d)'s CLaSS baseline on the GPU box's host cores: `rejection_sample(1 M)` the way the reference runs it - scikit-learn's
    GaussianMixture.sample + LogisticRegression.predict_proba per attribute + the accept test (/root/reference/density_modeling.py:50-60)
    - and the numpy oracle's Beam.py-order beam-5 / n-best-3 decode of 10 k z (sample_pipeline.py:129-139 decodes EVERY proposal) on ALL
    cores (one forked process per core, each with a single BLAS thread).  accepted/s = proposals/s x accept rate, proposals/s from the
    two per-z costs."""
    import multiprocessing as mp
    import sklearn.mixture
    from sklearn.linear_model import LogisticRegression
    from oracle import class_sampler as ocs
    P = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items() if not k.startswith("classifier")}
    _, cores, _logical = host_cpu()      # PHYSICAL cores (the training baseline states the same unit)
    K, D = Q._m.shape
    gm = sklearn.mixture.GaussianMixture(n_components=K, covariance_type="diag")
    gm.weights_, gm.means_, gm.covariances_ = Q._w, Q._m, Q._c
    gm.precisions_cholesky_ = 1.0 / np.sqrt(Q._c)
    coef, icpt, tgt = (t.cpu().numpy() for t in Q._dev_clf)
    clfs = []
    for i in range(len(tgt)):
        clf = LogisticRegression()
        clf.coef_, clf.intercept_, clf.classes_ = coef[i:i + 1], icpt[i:i + 1], np.array([0, 1])
        clfs.append((clf, int(tgt[i])))
    np.random.seed(0)
    t0 = time.perf_counter()
    z, _ = gm.sample(n_score)                                           # density_modeling.py:72-76 (mog.sample)
    accum = np.ones(n_score)
    for clf, target in clfs:                                            # :52-57: predict_proba of every attribute classifier
        accum *= clf.predict_proba(z)[:, target]
    acc = accum > np.random.uniform(size=n_score)                      # :58-59
    t_score = time.perf_counter() - t0
    z32 = z[:n_decode].astype(np.float32)
    c = np.zeros((n_decode, 2), np.float32)
    c[np.arange(n_decode), np.random.randint(0, 2, n_decode)] = 1
    # one process per core up to 64 (forking this process - it maps the GPU runtime and gigabytes of pinned memory - costs ~50 ms per
    # child, and below ~150 z per process the python start-up outweighs the decode)
    procs = max(1, min(cores, 64, n_decode // 150))
    bounds = np.linspace(0, n_decode, procs + 1).astype(int)
    _BEAM_JOB.update(P=P, z=z32, c=c)
    jobs = [(int(a), int(b)) for a, b in zip(bounds[:-1], bounds[1:]) if b > a]
    t0 = time.perf_counter()
    with mp.get_context("fork").Pool(procs) as pool:
        steps = sum(pool.map(_beam_chunk, jobs, chunksize=1))
    t_dec = time.perf_counter() - t0
    _BEAM_JOB.clear()
    z_per_s = 1.0 / (t_score / n_score + t_dec / n_decode)     # reference behaviour: every proposal is decoded
    return {"value": round(z_per_s * float(acc.mean()), 1), "unit": "accepted-samples/s", "cores": procs, "kind": "port",
            "sample": f"SURVEY 8(d): scikit-learn GaussianMixture.sample + LogisticRegression.predict_proba + accept test of {n_score} z "
                      f"({t_score:.2f} s, numpy / BLAS threads as installed) + oracle/decode.py beam-5 / n-best-3 of {n_decode} z on {procs} "
                      f"processes ({t_dec:.1f} s, {5 * steps / t_dec:.0f} decoder row-step evals/s); every proposal decoded, as "
                      f"sample_pipeline.py:129-139 does",
            "z_per_s": round(z_per_s, 1), "decoder_evals_per_s": round(5 * steps / t_dec, 1), "accept_rate": round(float(acc.mean()), 4)}


def class_bench(dev, N=1000000, cpu=True, rank=0, world=1):
    """BASELINE.json configs[3]: ONE sampling round of N proposals IN TOTAL through sample_pipeline.run_rounds - device GMM draw,
    LR scoring + accept test, beam-5 / n-best-3 decode (the reference decodes EVERY proposal), residue rows, de-duplication,
    the final pandas table - wall-clock, plus the accepted-only and greedy variants of the same round.  With world > 1 the
    round's rows are sharded over the ranks (N / world each, counter-based streams: the union is the single-rank round), every
    rank decodes its rows, the rows are all-gathered over RCCL and de-duplicated identically on every rank: strong scaling."""
    import logging
    import sample_pipeline as sp
    from cpg import dist as cdist
    from cpg import ops
    logging.getLogger('GenerationAPI').setLevel(logging.WARNING)
    m, Q, ds = class_setup(dev)
    N = N // (4 * world) * (4 * world)
    EVAL_FLOPS = 2.0 * 3 * 102 * (252 + 102) + 2.0 * 102 * 24    # one decoder row-step (221.5 kFLOP at config A)
    out = {}
    sp.run_rounds(m, ds, Q, 65536 // (4 * world) * (4 * world), 10 ** 9, max_rounds=1, sample_mode='beam')   # warm-up (code load, allocator)
    for tag, kw in (("beam5_all", dict(sample_mode='beam')), ("beam5_accepted_only", dict(sample_mode='beam', decode_accepted_only=True)),
                    ("greedy_all", dict(sample_mode='greedy'))):
        torch.cuda.synchronize()
        cdist.barrier()
        note("CLaSS variant " + tag)
        ops.PROFILE = []
        t0 = time.perf_counter()
        df, st = sp.run_rounds(m, ds, Q, N, 10 ** 9, max_rounds=1, return_stats=True, **kw)
        torch.cuda.synchronize()
        cdist.barrier()
        dt = time.perf_counter() - t0
        if world > 1:
            tmax = torch.tensor([dt], device=dev, dtype=torch.float64)
            cdist.allreduce_max(tmax)
            dt = float(tmax.item())
        prof, ops.PROFILE = ops.PROFILE, None
        kms = sum(e0.elapsed_time(e1) for _, e0, e1, _, _ in prof)
        launches = sum(l for _, _, _, l, _ in prof)
        r = {"proposals": st["proposed"], "decoded": st["decoded"], "accepted_unique": int(df['accept'].sum()), "unique": len(df),
             "wall_s": round(dt, 3), "accepted_per_s": round(float(df['accept'].sum()) / dt, 1),
             "proposals_per_s": round(st["proposed"] / dt, 1), "decoder_evals_per_s": round(st["decoder_evals"] / dt, 1),
             "decoder_evals": st["decoder_evals"], "decode_kernel_ms": round(kms, 2)}
        if kms > 0:
            ach = st["decoder_evals"] / world * EVAL_FLOPS / (kms * 1e-3) / 1e12     # this rank's kernel time, this rank's share of the evals
            r["roofline"] = {"bound": "mfma", "kernel": _cname("cpg_decode_fused_kernel_name", 1 if kw["sample_mode"] == "beam" else 0, 102, 5),
                             "achieved": round(ach, 2), "peak": round(PEAK_PAIR_TFLOPS, 1), "unit": "TFLOP/s", "frac": round(ach / PEAK_PAIR_TFLOPS, 4),
                             "frac_of_f32_mfma_peak": round(ach / PEAK_F32_MFMA_TFLOPS, 4),
                             "traffic": None, "avg_launch_us": round(kms * 1e3 / max(launches, 1), 1), "launches_timed": launches,
                             "flops_per_eval": EVAL_FLOPS, "pipe": "f16 MFMA x3 on f16-pair operands (f32-grade): 2500/3; W_hh fragments in registers, "
                             "state in LDS, nothing but ids leaves the CU (csrc/decode_fused.hip) - the kernel is bound by its VALU work (cell "
                             "nonlinearities, selection), not by the matrix pipe or HBM; algorithmic flops = live row-steps x (dense W_ih + W_hh + fc); "
                             "per-GPU rate (rank 0's kernels)"}
        out[tag] = r
    head = out["beam5_all"]
    wide = None
    if world == 1:
        wide = class_wide(dev)
    res = {"workload": f"BASELINE.json configs[3] on {world} GPU(s): {N} z proposals in total ({N // world} per GPU; synthetic GMM K=100), 2 LR heads, "
                       f"reference defaults z=100 / decoder h=102 / V=24 / T=25, c ~ Cat(.5,.5) per proposal, beam-5 decode of every proposal through "
                       f"sample_pipeline.run_rounds" + ("; rows all-gathered across the ranks and de-duplicated on the gathered set" if world > 1 else ""),
           "metric": "CLaSS accepted-samples/s", "value": head["accepted_per_s"], "unit": "accepted-samples/s", "n_gpus": world,
           "scaling": "strong", "decoder_evals_per_s": head["decoder_evals_per_s"], "roofline": head.get("roofline"), "variants": out}
    if wide is not None:
        res["config_b_width"] = wide
    if cpu and rank == 0:
        note("CLaSS cpu baseline")
        res["cpu_baseline"] = class_cpu_baseline(m, Q)
    return res


def class_wide(dev, Z=510, N=131072):
    """The CLaSS round at config-B width (z = 510, decoder h = 512, SURVEY 8d: 3.63 MFLOP per decoder row-step): no whole-loop kernel
    covers that width (W_hh alone is 4.7 MB of planes), so sample_G runs the per-step launch chain cpg_gru_step_fwd -> cpg_vocab_fc_fwd
    -> select (round-3 verdict: this path had no bench number).  One round of N proposals, greedy and beam-5 of every proposal."""
    import logging
    import sample_pipeline as sp
    from cpg import ops
    logging.getLogger('GenerationAPI').setLevel(logging.WARNING)
    m, Q, ds = class_setup(dev, Z=Z, enc_h=64)
    H = Z + 2
    EVAL_FLOPS = 2.0 * 3 * H * (150 + H + H) + 2.0 * H * 24
    out = {"workload": f"one CLaSS round of {N} proposals at z={Z} / decoder h={H} (config-B width), per-step decode launches", "flops_per_eval": EVAL_FLOPS}
    sp.run_rounds(m, ds, Q, 8192, 10 ** 9, max_rounds=1, sample_mode='greedy')
    from cpg import lib
    kname = _cname("cpg_gru_step_kernel_name", 0, 65536, H, 1, 0)
    wpeak = PEAK_PAIR_TFLOPS if kname.endswith(", 8>") else PEAK_SPLIT_TFLOPS   # the step kernel's product form (f16 pairs / bf16 triple)
    if lib().dll.cpg_gru_step_planes_ok(N, H) == 1 and not os.environ.get("CPG_NO_STEP_PLANES"):
        # round 5: the step runs on f16-pair plane images (cpg_gru_step_fwd_planes) - greedy rows N, beam rows N x 5
        kname, wpeak = "gru_step_fwd_planes_kernel", PEAK_PAIR_TFLOPS
    for tag, mode in (("greedy_all", "greedy"), ("beam5_all", "beam")):
        torch.cuda.synchronize()
        ops.PROFILE = []
        t0 = time.perf_counter()
        df, st = sp.run_rounds(m, ds, Q, N, 10 ** 9, max_rounds=1, return_stats=True, sample_mode=mode)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        prof, ops.PROFILE = ops.PROFILE, None
        kms = sum(e0.elapsed_time(e1) for fam, e0, e1, _, _ in prof if fam == "decode_step_chain")
        steps = sum(l for fam, _, _, l, _ in prof if fam == "decode_step_chain")
        ach = st["decoder_evals"] * EVAL_FLOPS / (kms * 1e-3) / 1e12 if kms > 0 else 0.0
        out[tag] = {"wall_s": round(dt, 3), "accepted_per_s": round(float(df['accept'].sum()) / dt, 1), "decoder_evals": st["decoder_evals"],
                    "decoder_evals_per_s": round(st["decoder_evals"] / dt, 1), "decode_chain_ms": round(kms, 2), "chain_steps": steps,
                    "roofline": {"bound": "mfma", "kernel": kname, "achieved": round(ach, 2),
                                 "peak": round(wpeak, 1), "unit": "TFLOP/s", "frac": round(ach / wpeak, 4),
                                 "note": "algorithmic flops of the live row-steps (dense W_ih + W_hh + fc) over the time of the per-step "
                                         "chain (step kernel + vocabulary projection + selection)"}}
    del m
    torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    main()
    if _PROBE_HUNG:   # a probe thread is stuck inside RCCL: do not wait for it at interpreter shutdown
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(0)
