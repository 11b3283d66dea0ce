#!/usr/bin/env python3
"""Headline benchmark: DiT denoising steps/sec, CogVideoX-5B To2V 720x480 (BASELINE.json configs[1] shape).

One "step" = the body of the reference's per-GPU FIFO worker (cogvideo_sampling_mp_fifo.py:491-550): a
CFG-batched (B=2) DiT forward over one 13-latent-frame window (226 text + 17 550 video + 480 condensed tokens,
42 layers, D=3072) + CFG combine + 13 per-frame DPM-solver++ updates.  Synthetic latents / embeddings and
random-init weights of the real architecture (no checkpoints offline).  Inputs are resident in HBM when the
timed region starts.

N > 1 (one rank per GPU, RCCL; launched by torch.distributed.run, or — when RANK is not in the environment — by bench.py itself
through tokensgen_amd.runtime.launch): every rank runs its own window of the same
FIFO iteration (weak scaling, windows are independent) and the window outputs are exchanged with ONE
all_gather per step — the same message tokensgen_amd/fifo.py sends (2 x 13 frames per window + the rank's
failure flag).

Prints ONE JSON line (rank 0).  A plain run sets up, warms up, times `--steps` steps and prints the headline (`value`, `ms_per_step`, ...);
`--full` adds everything else on the record (per-kernel and roofline times, the other attention path, power and clock, the zero-operand
control, the VAE and training sub-records, the CPU baseline) and writes the full record to the detail file.  `--dump-outputs DIR` saves what
the last timed step returned, as float32 .npy; the inputs are seeded, so equal arguments give equal inputs.
"""
import argparse
import contextlib
import json
import os
import re
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FLOP_PER_STEP = 776.0e12          # 42 x 9.237 TFLOP/block/sample x 2 + embed/out
PEAK_BF16 = 2.5e15                # MI355X dense bf16 MFMA peak (MI355X_MICROARCH.md)
# dominant kernel = fused main attention (SDPA#1 + SDPA#2 of the To2V processor), per launch (B=2):
N1, NP, D_MODEL = 17776, 480, 3072
# + the vip-query attention (SDPA#3), whose workgroups ride in the same launch (tg_attention_fwd_multi)
PMC_SUMMARY = "r6_pmc_summary.json"     # committed rocprofv3 PMC passes the `traffic` figure is read from
BWD_PMC_SUMMARY = "r6_attention_bwd_pmc.json"   # likewise for the training sub-record's dominant kernel (tools/profile_attn_bwd.sh)
ATTN_FLOP_PER_LAUNCH = 2 * (4.0 * N1 * N1 * D_MODEL + 4.0 * N1 * NP * D_MODEL + 4.0 * NP * (N1 + NP) * D_MODEL)


def build_model(device, layers):
    from tokensgen_amd.transformer import CogVideoXTransformer3DModel
    m = CogVideoXTransformer3DModel(num_attention_heads=48, attention_head_dim=64, num_layers=layers, time_embed_dim=512,
                                    text_embed_dim=4096, use_rotary_positional_embeddings=True, device=device)
    m.set_vip_layers(None, length=480, func_type="1", scale=[0.6],
                     resampler_params=dict(output_dim=3072, num_height_queries=8, num_width_queries=12, num_temporal_queries=4))
    g = torch.Generator(device=device).manual_seed(1234)
    for name, t in m._fused.items():       # random init at the real shapes, straight into the fused storages
        if t.dim() == 2 and t.shape[0] > 8:
            t.copy_(torch.randn(t.shape, generator=g, device=device, dtype=torch.float32) * 0.02)
        elif name.endswith(("ln", "qknorm", "vln", "vqknorm")):
            t.copy_(torch.randn(t.shape, generator=g, device=device, dtype=torch.float32) * 0.05)
            t[0::2] += 1.0
        else:
            t.copy_(torch.randn(t.shape, generator=g, device=device, dtype=torch.float32) * 0.02)
    return m


def _cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def _physical_cores():
    """Distinct (physical id, core id) pairs of /proc/cpuinfo restricted to this process's affinity; falls back to os.cpu_count()."""
    try:
        allowed = os.sched_getaffinity(0)
        cores, cpu, phys = set(), None, None
        with open("/proc/cpuinfo") as f:
            for line in f:
                k, _, v = line.partition(":")
                k, v = k.strip(), v.strip()
                if k == "processor":
                    cpu = int(v)
                elif k == "physical id":
                    phys = v
                elif k == "core id" and cpu in allowed:
                    cores.add((phys, v))
        if cores:
            return len(cores)
    except (OSError, ValueError, AttributeError):
        pass
    return os.cpu_count() or 1


class PowerSampler:
    """Socket power and shader clock of ONE GPU sampled by a host thread while a timed region runs (the power-cap reading of the
    roofline fractions belongs on the driver's record).  No GPU work: sysfs hwmon files of the device (power1_average / power1_input in microwatts,
    power1_cap, freq1_input in Hz; the starred line of pp_dpm_sclk as a second clock source), else the amdsmi python binding that ships with ROCm, else one
    rocm-smi subprocess per sample.  `summary()` says which source answered; every figure is None when none did — never a guess."""

    def __init__(self, device_index=0, period_s=0.05):
        self.period, self.samples, self._stop, self._thread = period_s, [], False, None
        self.source, self.cap_W = None, None
        self._smi, self._idx, self._viol0, self._viol1, self.pci = None, device_index, None, None, None
        self._read = self._pick(device_index)

    # -- sources --------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _num(path):
        try:
            with open(path) as f:
                return float(f.read().strip().split()[0])
        except (OSError, ValueError, IndexError):
            return None

    def _pick(self, idx):
        import glob
        want = None
        try:
            pr = torch.cuda.get_device_properties(idx)
            want = "%04x:%02x:%02x" % (getattr(pr, "pci_domain_id", 0), pr.pci_bus_id, pr.pci_device_id)
        except Exception:  # noqa: BLE001
            pass
        cands = []
        for c in sorted(glob.glob("/sys/class/drm/card[0-9]*/device")):
            hw = sorted(glob.glob(os.path.join(c, "hwmon", "hwmon*")))
            if hw:
                cands.append((c, hw[0], os.path.basename(os.path.realpath(c)).lower()))
        pick = next(((c, hw) for c, hw, addr in cands if want and addr.startswith(want)), None)
        if pick is None and len(cands) == 1:
            pick = cands[0][:2]
        self.pci = want
        if pick is not None:
            c, hw = pick
            pfile = next((p for p in (os.path.join(hw, "power1_average"), os.path.join(hw, "power1_input")) if self._num(p) is not None), None)
            ffile = os.path.join(hw, "freq1_input") if self._num(os.path.join(hw, "freq1_input")) is not None else None
            dpm = os.path.join(c, "pp_dpm_sclk") if os.path.exists(os.path.join(c, "pp_dpm_sclk")) else None
            if pfile or ffile or dpm:
                cap = self._num(os.path.join(hw, "power1_cap"))
                self.cap_W = cap / 1e6 if cap else None
                self.source = "sysfs:" + hw

                def read():
                    p = self._num(pfile) if pfile else None
                    f = self._num(ffile) if ffile else None
                    mhz = f / 1e6 if f else None
                    if mhz is None and dpm:
                        try:
                            with open(dpm) as fh:
                                for line in fh:
                                    if "*" in line:
                                        mhz = float(re.search(r"(\d+)\s*mhz", line.lower()).group(1))
                        except (OSError, AttributeError, ValueError):
                            pass
                    return (p / 1e6 if p else None, mhz)
                if any(v is not None for v in read()):
                    return read
        try:
            sys.path.append("/opt/rocm/share/amd_smi")
            import amdsmi
            amdsmi.amdsmi_init()
            h = amdsmi.amdsmi_get_processor_handles()[idx]
            try:
                self.cap_W = float(amdsmi.amdsmi_get_power_cap_info(h)["power_cap"]) / 1e6
            except Exception:  # noqa: BLE001
                pass
            self.source = "amdsmi"

            def read():
                p = mhz = None
                try:
                    pi = amdsmi.amdsmi_get_power_info(h)
                    p = float(pi.get("current_socket_power") or pi.get("average_socket_power") or 0) or None
                except Exception:  # noqa: BLE001
                    pass
                try:
                    mhz = float(amdsmi.amdsmi_get_clock_info(h, amdsmi.AmdSmiClkType.GFX)["clk"]) or None
                except Exception:  # noqa: BLE001
                    pass
                return (p, mhz)
            if any(v is not None for v in read()):
                return read
        except Exception:  # noqa: BLE001
            pass
        import shutil
        import subprocess
        if shutil.which("rocm-smi"):
            self.source, self.period = "rocm-smi", max(self.period, 0.25)

            def read():
                try:
                    out = subprocess.run(["rocm-smi", "-d", str(idx), "--showclocks", "--showpower", "--json"], capture_output=True, text=True, timeout=5).stdout
                    d = next(iter(json.loads(out).values()))
                    p = next((float(v) for k, v in d.items() if "power" in k.lower() and "(w)" in k.lower()), None)
                    m = next((re.search(r"(\d+)", v) for k, v in d.items() if k.lower().startswith("sclk")), None)
                    return (p, float(m.group(1)) if m else None)
                except Exception:  # noqa: BLE001
                    return (None, None)
            return read
        self.source = None
        return lambda: (None, None)

    # -- which limiter held the clock down (VERDICT r5 weak #4a: read, not asserted) ------------------------------------------------
    def _violations(self):
        """Accumulated throttler residencies of the device (amdsmi violation status: counts of firmware intervals spent on each limiter — package power PPT,
        socket / VR / HBM thermal, PROCHOT — beside the count of all intervals), or the gpu_metrics residency accumulators, or None.  Two snapshots around a
        timed region give the fraction of the region each limiter was active; nothing is derived from power or clock."""
        try:
            if self._smi is None:
                sys.path.append("/opt/rocm/share/amd_smi")
                import amdsmi
                try:
                    amdsmi.amdsmi_init()
                except Exception:  # noqa: BLE001  (already initialised by _pick)
                    pass
                hs = amdsmi.amdsmi_get_processor_handles()
                h = None
                for cand in hs:
                    try:
                        bdf = amdsmi.amdsmi_get_gpu_device_bdf(cand).lower()
                        if self.pci and bdf.startswith(self.pci):
                            h = cand
                    except Exception:  # noqa: BLE001
                        pass
                if h is None:
                    h = hs[self._idx] if len(hs) > self._idx else hs[0]
                self._smi = (amdsmi, h)
            amdsmi, h = self._smi
        except Exception:  # noqa: BLE001
            self._smi = False
            return None
        if not self._smi:
            return None
        num = lambda v: float(v) if isinstance(v, (int, float)) else None

        def leaves(v):
            if isinstance(v, (list, tuple)):
                vals = [x for x in (leaves(u) for u in v) if x is not None]
                return sum(vals) if vals else None
            return num(v)
        try:
            v = amdsmi.amdsmi_get_violation_status(h)
            snap = {"source": "amdsmi_get_violation_status", "intervals": num(v.get("acc_counter")), "ppt": num(v.get("acc_ppt_pwr")),
                    "socket_thermal": num(v.get("acc_socket_thrm")), "vr_thermal": num(v.get("acc_vr_thrm")), "hbm_thermal": num(v.get("acc_hbm_thrm")),
                    "prochot": num(v.get("acc_prochot_thrm")),
                    # per-XCD "shader clock below the host limit because of power / of temperature" accumulators (gpu_metrics 1.8 xcp_stats), summed over the XCDs
                    "gfx_clk_below_host_limit_pwr": leaves(v.get("acc_gfx_clk_below_host_limit_pwr")),
                    "gfx_clk_below_host_limit_thm": leaves(v.get("acc_gfx_clk_below_host_limit_thm"))}
            if snap["intervals"] is not None:
                return snap
        except Exception:  # noqa: BLE001
            pass
        try:
            m = amdsmi.amdsmi_get_gpu_metrics_info(h)
            snap = {"source": "amdsmi_get_gpu_metrics_info", "intervals": num(m.get("accumulation_counter")), "ppt": num(m.get("ppt_residency_acc")),
                    "socket_thermal": num(m.get("socket_thm_residency_acc")), "vr_thermal": num(m.get("vr_thm_residency_acc")),
                    "hbm_thermal": num(m.get("hbm_thm_residency_acc")), "prochot": num(m.get("prochot_residency_acc")),
                    "throttle_status": m.get("throttle_status") if isinstance(m.get("throttle_status"), int) else None}
            if snap["intervals"] is not None or snap["ppt"] is not None:
                return snap
        except Exception:  # noqa: BLE001
            pass
        return None

    def limiter(self):
        """{limiter: fraction of the sampled region it was active} + the name of the largest, from the two snapshots taken by __enter__ / __exit__; None when the box offers no source."""
        a, b = self._viol0, self._viol1
        if not a or not b:
            return None
        names = ("ppt", "socket_thermal", "vr_thermal", "hbm_thermal", "prochot", "gfx_clk_below_host_limit_pwr", "gfx_clk_below_host_limit_thm")
        dn = (b["intervals"] - a["intervals"]) if a.get("intervals") is not None and b.get("intervals") is not None else None
        out = {"source": b["source"], "intervals": dn}
        frac = {}
        for n in names:
            if a.get(n) is not None and b.get(n) is not None:
                d = b[n] - a[n]
                frac[n] = (d / dn) if dn else d
        out["active_frac" if dn else "active_counts"] = {k: round(v, 4) for k, v in frac.items()}
        main = {k: v for k, v in frac.items() if not k.startswith("gfx_clk")}      # the per-XCD sums are reported, not ranked
        top = max(main, key=main.get) if main else None
        # named only when it was active for at least 5 % of the region (a handful of intervals at the start of a burst is not "the limiter")
        out["limiter"] = (top if (frac.get(top, 0) >= 0.05 if dn else frac.get(top, 0) > 0) else "none") if top else None
        return out

    # -- sampling -------------------------------------------------------------------------------------------------------------
    def __enter__(self):
        import threading
        self.samples, self._stop = [], False
        self._viol0, self._viol1 = self._violations(), None

        def loop():
            while not self._stop:
                self.samples.append(self._read())
                time.sleep(self.period)
        self._thread = threading.Thread(target=loop, daemon=True)
        self._thread.start()
        return self

    def __exit__(self, *exc):
        self._viol1 = self._violations()
        self._stop = True
        self._thread.join(timeout=10)
        return False

    def summary(self):
        pw = [p for p, _ in self.samples if p is not None]
        ck = [c for _, c in self.samples if c is not None]
        mean = lambda v: (sum(v) / len(v)) if v else None
        return {"power_W_mean": mean(pw), "power_W_max": max(pw) if pw else None, "power_cap_W": self.cap_W, "sclk_MHz_mean": mean(ck),
                "sclk_MHz_min": min(ck) if ck else None, "sclk_MHz_max": max(ck) if ck else None, "samples": len(self.samples), "source": self.source, "pci": getattr(self, "pci", None), "limiter": self.limiter()}


def cpu_baseline(seconds_budget=150.0):
    """SURVEY §8(d) protocol: the oracle (CPU restatement of the reference, validated against it) timed on this box's host cores on a
    bounded sample of the same workload — ONE full-width block forward (B=1) of the 84 a step needs — bf16 and fp32, 1 warm-up + up to 3
    timed runs each (median; fewer runs only if `seconds_budget` runs out), on the thread count that is fastest among {physical cores / 2,
    physical cores, logical cores} in a short GEMM probe (256 logical threads oversubscribed the round-1 baseline 3x)."""
    from oracle import dit_ref as O
    logical = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    physical = min(_physical_cores(), logical)
    t_start = time.perf_counter()
    a, b = torch.randn(4096, 3072).bfloat16(), torch.randn(3072, 3072).bfloat16()
    probe = {}
    for n in sorted({max(1, physical // 2), physical, logical}):
        torch.set_num_threads(n)
        a @ b
        t0 = time.perf_counter()
        for _ in range(3):
            a @ b
        probe[n] = (time.perf_counter() - t0) / 3
    threads = min(probe, key=probe.get)
    torch.set_num_threads(threads)
    cfg = dict(num_attention_heads=48, attention_head_dim=64, num_layers=1, time_embed_dim=512)
    sd32 = {k: v for k, v in O.make_state_dict(cfg, n_vip_dim=3072, seed=500).items() if k.startswith("transformer_blocks.0.")}
    g = torch.Generator().manual_seed(501)
    hid, enc, temb = torch.randn(1, 17550, 3072, generator=g), torch.randn(1, 706, 3072, generator=g), torch.randn(1, 13, 512, generator=g)
    f32 = np.float32
    rope = O.rope_3d(64, np.arange(13, dtype=f32), np.arange(30, dtype=f32), np.arange(45, dtype=f32))
    crope = O.rope_3d(64, np.linspace(1000, 1016.25, 5, dtype=f32), np.linspace(0, 30, 8, endpoint=False, dtype=f32),
                      np.linspace(0, 45, 12, endpoint=False, dtype=f32))
    res = {}
    for name, dt_ in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
        sd = {k: v.to(dt_) for k, v in sd32.items()}
        args = (sd, "transformer_blocks.0", hid.to(dt_), enc.to(dt_), temb.to(dt_), 48, 480, [0.6], rope, rope, crope)
        times = []
        with torch.no_grad():
            O.block_forward(*args)                                   # warm-up
            # bf16 gets the first 60 % of the budget, fp32 the rest; always at least one timed run
            limit = t_start + seconds_budget * (0.6 if name == "bf16" else 1.0)
            while len(times) < 3 and (not times or time.perf_counter() + times[-1] < limit):
                t0 = time.perf_counter()
                O.block_forward(*args)
                times.append(time.perf_counter() - t0)
        res[name] = (sorted(times)[len(times) // 2], len(times))
    med, n = res["bf16"]
    return {"value": 1.0 / (med * 84.0), "unit": "steps/s", "cores": threads, "kind": "port",
            "sample": f"1 full-width CogVideoXBlock forward (B=1) of the 84 per step, extrapolated x84: bf16 median {med:.2f} s over {n} runs, "
                      f"fp32 median {res['fp32'][0]:.2f} s over {res['fp32'][1]} runs (1 warm-up each)",
            "fp32_value": 1.0 / (res["fp32"][0] * 84.0), "cpu_model": _cpu_model(), "physical_cores": physical, "logical_cores": logical,
            "threads_probe_s": {str(k): round(v, 4) for k, v in probe.items()}}


# To2V training micro-step (B = 2), algorithmic transformer flops per layer: forward 18.47 T (QKV 2.013 + vip QKV over all rows 2.067 + attention 8.19 + out 0.689 + FF 5.513)
# + attention backward 2.5 x 8.19 = 20.48 T + dgrad of the same five linears 10.28 T + wgrad of vip_to_{q,k,v} 2.067 T; x 42 layers
TRAIN_FLOP_PER_MICRO_STEP = 776.0e12 + 860.0e12 + 431.8e12 + 86.8e12
VAE_FLOP = {"decode": 3.1e14, "encode": 1.5e14}     # untiled algorithmic count per 49-frame clip; executed = x1.40 (9-tile overlap)


def vae_record(device, reps=3):
    """BASELINE config 4 (outside the timed DiT region): 3-D causal VAE decode [1,16,13,60,90] -> [1,3,49,480,720] and encode back,
    tiling + slicing on like the pipeline, random weights at the real widths.  Wall seconds = best of `reps` after one warm-up (the first repeat captures the tile graphs)."""
    from tokensgen_amd.vae import AutoencoderKLCogVideoX
    vae = AutoencoderKLCogVideoX(device=device).init_random(seed=1)
    vae.enable_tiling(); vae.enable_slicing()
    g = torch.Generator(device=device).manual_seed(0)
    z = (torch.randn(1, 16, 13, 60, 90, generator=g, device=device) / 1.15258426).to(torch.bfloat16)
    x = (torch.rand(1, 3, 49, 480, 720, generator=g, device=device) * 2 - 1).to(torch.bfloat16)
    out = {"workload": "AutoencoderKLCogVideoX 49x480x720 (13x60x90 latent), 9 spatial tiles x 6 temporal batches, bf16", "peak_TFLOPs": PEAK_BF16 / 1e12}
    for name, fn in (("decode", lambda: vae.decode(z).sample), ("encode", lambda: vae.encode(x).latent_dist.parameters)):
        y = fn(); torch.cuda.synchronize()
        best = float("inf")
        ps = PowerSampler(device.index or 0, period_s=0.02)        # the convolutions are MFMA kernels under the same socket power cap as the DiT: on the record
        with ps:
            for _ in range(reps):
                t0 = time.perf_counter(); y = fn(); torch.cuda.synchronize(); best = min(best, time.perf_counter() - t0)
        pw = ps.summary()
        out[name] = {"seconds": best, "algorithmic_TFLOPs": VAE_FLOP[name] / best / 1e12, "executed_TFLOPs": 1.4 * VAE_FLOP[name] / best / 1e12,
                     "frac_of_peak_algorithmic": VAE_FLOP[name] / best / PEAK_BF16, "frac_of_peak_executed": 1.4 * VAE_FLOP[name] / best / PEAK_BF16,
                     "out_shape": list(y.shape), "finite": bool(torch.isfinite(y).all()), "power_W_mean": pw["power_W_mean"], "sclk_MHz_mean": pw["sclk_MHz_mean"],
                     "sclk_MHz_min": pw["sclk_MHz_min"], "sclk_MHz_max": pw["sclk_MHz_max"], "limiter": pw["limiter"],
                     "frac_of_peak_executed_at_measured_clock": (1.4 * VAE_FLOP[name] / best / (PEAK_BF16 * pw["sclk_MHz_mean"] / 2400.0)) if pw["sclk_MHz_mean"] else None}
    del vae
    torch.cuda.empty_cache()
    return out


def run_e2e(a, rank, world, device, dist):
    """--mode e2e: ONE full To2V run on synthetic inputs — the 52-step base stage on chunk 0 (CFG-parallel over ranks 0/1 when world >= 2),
    the FIFO stage over `--chunks` clips INCLUDING the ramp (windows dealt round-robin to the ranks, one all_gather per iteration), and the
    chunk-sharded VAE decode with its all_gather of frames.  value = DiT window-forwards / wall / N (steps/s/GPU end to end); the base stage's
    scalar-timestep forwards count as window-forwards (same shape)."""
    from tokensgen_amd import fifo as F
    from tokensgen_amd.pipeline import MPFIFOVideoIPAdapterCogVideoXPipeline
    from tokensgen_amd.scheduler import CogVideoXDPMScheduler
    from tokensgen_amd.vae import AutoencoderKLCogVideoX
    model = build_model(device, a.layers)
    sched = CogVideoXDPMScheduler(prediction_type="v_prediction", rescale_betas_zero_snr=True, snr_shift_scale=1.0, timestep_spacing="trailing")
    vae = AutoencoderKLCogVideoX(device=device).init_random(seed=1)
    vae.enable_tiling(); vae.enable_slicing()
    pipe = MPFIFOVideoIPAdapterCogVideoXPipeline(model, sched, vae=vae)
    g = torch.Generator(device=device).manual_seed(42)           # same inputs on every rank (the reference ships them to its workers)
    bf = torch.bfloat16
    pe = (torch.randn(1, 226, 4096, generator=g, device=device) * 0.1).to(bf)
    ne = (torch.randn(1, 226, 4096, generator=g, device=device) * 0.1).to(bf)
    emb = torch.nn.functional.layer_norm(torch.randn(1, 4 * a.chunks, 8, 12, 3072, generator=g, device=device), (3072,))
    emb = emb.permute(0, 1, 4, 2, 3).to(bf).contiguous()         # [1, 4*chunks, 3072, 8, 12] as the T2To stage / Resampler hands it over
    t_t2to, t2to_tokens = None, None
    if a.mode == "gen":
        # gen.yaml (BASELINE config 3): the condensed tokens come from the T2To stage — a second, patch-1 CogVideoX-5B DiT denoising
        # [1, 4*chunks, 16, 8, 12] token latents over 52 steps with dynamic CFG, then de-normalisation + PCA inverse (pipeline_cogvideox_t2to.py:768-904).
        # Every rank runs it (it is not sharded in the reference either: infer_cogvideo_mp_fifo.py runs it before the workers start).
        from tokensgen_amd.pca import PCA
        from tokensgen_amd.pipeline_t2to import LongVGenCogVideoXPipeline
        from tokensgen_amd.transformer import CogVideoXTransformer3DModel
        m2 = CogVideoXTransformer3DModel(num_attention_heads=48, attention_head_dim=64, num_layers=a.layers, time_embed_dim=512, text_embed_dim=4096,
                                         patch_size=1, use_rotary_positional_embeddings=True, device=device)
        g2 = torch.Generator(device=device).manual_seed(4321)
        for name, t in m2._fused.items():
            t.copy_(torch.randn(t.shape, generator=g2, device=device, dtype=torch.float32) * 0.02)
            if name.endswith(("ln", "qknorm")):
                t[0::2] += 1.0
        sched2 = CogVideoXDPMScheduler(prediction_type="v_prediction", rescale_betas_zero_snr=True, snr_shift_scale=1.0, timestep_spacing="trailing")
        pipe2 = LongVGenCogVideoXPipeline(m2, sched2)
        cg = torch.Generator().manual_seed(2)
        pca = PCA()
        qm, _ = torch.linalg.qr(torch.randn(3072, 16, generator=cg))
        pca.register_buffer("mean_", torch.randn(1, 3072, generator=cg) * 0.1); pca.register_buffer("components_", qm.t().contiguous())
        kw2 = dict(prompt_embeds=pe.cpu().float(), negative_prompt_embeds=ne.cpu().float(), height=8, width=12, num_frames_per_chunk=4, num_chunks=a.chunks,
                   use_dynamic_cfg=True, guidance_scale=6.0, longvgen_mean=torch.randn(1, 16, generator=cg), longvgen_std=torch.rand(1, 16, generator=cg) + 0.5,
                   longvgen_pca=pca)
        pipe2(num_inference_steps=1, generator=torch.Generator().manual_seed(3), **kw2)          # warm-up (workspace, tables)
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        t0g = time.perf_counter()
        emb = pipe2(num_inference_steps=52, generator=torch.Generator().manual_seed(3), **kw2).frames.to(bf).contiguous()
        torch.cuda.synchronize()
        t_t2to, t2to_tokens = time.perf_counter() - t0g, 226 + 4 * a.chunks * 96
        assert emb.shape == (1, 4 * a.chunks, 3072, 8, 12) and torch.isfinite(emb).all()
        del pipe2, m2
        torch.cuda.empty_cache()
    counts = {"fifo": 0}
    orig_plan = F.window_plan

    def counting_plan(qs, nf=13, num_partitions=4):
        plan = orig_plan(qs, nf, num_partitions)
        counts["fifo"] += len(plan)
        return plan
    F.window_plan = counting_plan

    def fence():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier(); torch.cuda.synchronize()
    # checkpoints inside the FIFO loop (nothing may grow or drift over the 351 iterations of gen.yaml): device memory, a checksum of the
    # queue, wall time and window count at iterations 0, 100, 200, ..., last.  One host sync per checkpoint (a handful per run), nothing on the other iterations
    ckpt = []

    def hook(i, n_iter, lat, x0q):
        if i % 100 == 0 or i == n_iter - 1:
            lf = lat.float()
            ckpt.append({"iteration": i, "of": n_iter, "seconds_since_start": None, "window_forwards_so_far": counts["fifo"],
                         "queue_sum": float(lf.sum()), "queue_abs_mean": float(lf.abs().mean()), "queue_finite": bool(torch.isfinite(lf).all()),
                         "x0_abs_mean": float(x0q.float().abs().mean()),
                         "mem_allocated_GB": torch.cuda.memory_allocated() / 2 ** 30, "mem_max_allocated_GB": torch.cuda.max_memory_allocated() / 2 ** 30,
                         "mem_reserved_GB": torch.cuda.memory_reserved() / 2 ** 30})
            torch.cuda.synchronize()
            ckpt[-1]["seconds_since_start"] = time.perf_counter() - t0
    fence()
    power = PowerSampler(device.index or 0, period_s=0.5)
    power.__enter__()
    t0 = time.perf_counter()
    base = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, image_embeddings=emb, num_chunks=a.chunks, num_inference_steps=52,
                guidance_scale=6.0, video_ipadapter_scale=[0.6], output_type="pt")
    fence(); t_base = time.perf_counter() - t0
    orig, video, _ = F.cogvideo_fifo_mp_v2([pipe], base, noise_seed=7, iteration_hook=hook)
    fence(); dt = time.perf_counter() - t0
    power.__exit__()
    power = power.summary()
    # steady-state rate between the first and the last checkpoint (ramp and decode excluded), for comparison with the window benchmark
    steady = None
    if len(ckpt) >= 2 and ckpt[-1]["seconds_since_start"] > ckpt[0]["seconds_since_start"]:
        steady = (ckpt[-1]["window_forwards_so_far"] - ckpt[0]["window_forwards_so_far"]) / (ckpt[-1]["seconds_since_start"] - ckpt[0]["seconds_since_start"]) / world
    if t_t2to is not None:
        dt += t_t2to                                              # the whole generation: T2To stage + To2V
    F.window_plan = orig_plan
    if dist is not None:
        tm = torch.tensor([dt], device=device, dtype=torch.float64)
        dist.all_reduce(tm, op=dist.ReduceOp.MAX)
        dt = float(tm.item())
    if rank == 0:
        fwd = 52 + counts["fifo"]
        print(json.dumps({
            "metric": "DiT denoising steps/sec/GPU END TO END (" + ("T2To token stage + " if t_t2to is not None else "") +
                      "base stage + FIFO incl. ramp + sharded VAE decode), CogVideoX-5B To2V 720x480",
            "value": fwd / dt / world, "unit": "steps/s/GPU", "n_gpus": world, "steps": fwd, "warmup": 0, "ms_per_step": 1e3 * dt / fwd,
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "bf16",
            "data": "synthetic embeddings, random-init weights at CogVideoX-5B shapes",
            "config": {"workload": f"To2V end to end, {a.chunks} clip(s) of 49 frames: 52 base steps + {counts['fifo']} FIFO window-forwards "
                                   f"+ VAE decode of {a.chunks + 1} clips", "layers": a.layers, "chunks": a.chunks},
            "seconds": {"total": dt, "base_stage": t_base, "fifo_and_decode": dt - t_base - (t_t2to or 0.0), "t2to_stage": t_t2to},
            "t2to": None if t_t2to is None else {"tokens": t2to_tokens, "steps": 52, "ms_per_cfg_step": 1e3 * t_t2to / 52},
            "fifo_steps_per_s_per_gpu_between_checkpoints": steady, "checkpoints": ckpt,
            "peak_mem_GB": torch.cuda.max_memory_allocated() / 2 ** 30, "power_W_mean": power["power_W_mean"], "power_cap_W": power["power_cap_W"],
            "sclk_MHz_mean": power["sclk_MHz_mean"],
            "frames_out": list(video.shape), "finite": bool(torch.isfinite(video).all())}))


def build_resampler_sd(device):
    """Random-init Resampler at the yaml's shapes (cogvideo_5b_vaevip_4x8x12_to2v.yaml resampler_params) under the reference's key names."""
    dim, depth, heads, dh, emb, out, mult = 3072, 4, 16, 64, 3072, 3072, 4
    inner, nq = heads * dh, 4 * 8 * 12
    g = torch.Generator(device=device).manual_seed(4321)
    bf = torch.bfloat16
    rn = lambda *s, sc=0.02: (torch.randn(*s, generator=g, device=device, dtype=torch.float32) * sc).to(bf)
    ln = lambda n: (1 + rn(n, sc=0.05).float()).to(bf)
    sd = {"latents": rn(1, nq, dim, sc=dim ** -0.5), "proj_in.weight": rn(dim, emb), "proj_in.bias": rn(dim), "proj_out.weight": rn(out, dim),
          "proj_out.bias": rn(out), "norm_out.weight": ln(out), "norm_out.bias": rn(out, sc=0.05)}
    for i in range(depth):
        p, f = f"layers.{i}.0", f"layers.{i}.1"
        for n, w in (("norm1", dim), ("norm2", dim), ("norm_q", dh), ("norm_k", dh)):
            sd[f"{p}.{n}.weight"], sd[f"{p}.{n}.bias"] = ln(w), rn(w, sc=0.05)
        sd[p + ".to_q.weight"], sd[p + ".to_kv.weight"], sd[p + ".to_out.weight"] = rn(inner, dim), rn(2 * inner, dim), rn(dim, inner)
        sd[f + ".net.0.proj.weight"], sd[f + ".net.0.proj.bias"] = rn(dim * mult, dim), rn(dim * mult)
        sd[f + ".net.2.weight"], sd[f + ".net.2.bias"] = rn(dim, dim * mult), rn(dim)
    return sd, depth, heads


def run_train(a, rank, world, device, dist):
    """--mode train: prints train_measure()'s record as the one JSON line (rank 0)."""
    rec = train_measure(a, rank, world, device, dist)
    if rank == 0:
        print(json.dumps(rec))


def train_measure(a, rank, world, device, dist, ckpt_leg_steps=0):
    """BASELINE config 5 (`--mode train`, and the `train` sub-record of the default run): To2V training micro-steps at the yaml's shapes — per_gpu_batch_size 2, 13 latent frames of 60 x 90, 226 text
    tokens, the Resampler (trainable) over two 13-frame chunks -> 480 vip tokens, transformer forward with per-block checkpointing, v-prediction
    loss, backward with recompute, gradient accumulation over `--accum` micro-steps, then bucketed RCCL all-reduce (N > 1), clip, AdamW.
    A "step" is one micro-step (one micro-batch per rank); the timed region holds exactly `--steps` of them, optimizer steps included when
    they fall inside.  value = samples / s over all ranks.  Not in the timed region (as in the reference's throughput-relevant part): VAE encode
    and T5 run under no_grad before the micro-step and are BASELINE config 4 / out of scope respectively."""
    from tokensgen_amd import kernels as K
    from tokensgen_amd import optim, train
    from tokensgen_amd import rope as R
    from tokensgen_amd.scheduler import CogVideoXDPMScheduler
    bf = torch.bfloat16
    model = build_model(device, a.layers)
    sd = {k: v.detach() for k, v in model.state_dict().items()}
    tr = train.To2VTrainer(sd, 48, a.layers, patch_size=2, vip_scale=1.0)
    rsd, depth, heads = build_resampler_sd(device)
    rt = train.ResamplerTrainer(rsd, depth=depth, heads=heads)
    params = {k: sd[k] for k in tr.trainable}
    params.update({"resampler." + k: v for k, v in rsd.items()})
    arena = optim.ParamArena(params, optim.arena_order(list(params), a.layers), device)
    tr.use_arena(arena); rt.use_arena(arena)
    del params
    n_clip = arena.prefix_elems(lambda n: not n.startswith("resampler."))
    opt = optim.AdamW(arena, lr=2e-4, betas=(0.9, 0.95), eps=1e-8, weight_decay=1e-4, max_grad_norm=1.0, clip_elems=n_clip)
    sync = optim.GradSync(arena.grad, bucket_elems=64 * 1024 * 1024) if dist is not None else None
    sched = CogVideoXDPMScheduler(prediction_type="v_prediction", rescale_betas_zero_snr=True, snr_shift_scale=1.0, timestep_spacing="trailing")
    step = train.To2VTrainStep(tr, arena, opt, sched.alphas_cumprod.to(torch.float32), accumulation_steps=a.accum, sync=sync, resampler=rt)
    g = torch.Generator(device=device).manual_seed(7 + rank)
    B, nf, C, H, W = 2, 13, 16, 60, 90
    x0, noise = (torch.randn(B, nf, C, H, W, generator=g, device=device, dtype=torch.float32).to(bf) for _ in range(2))
    text = (torch.randn(B, 226, 4096, generator=g, device=device, dtype=torch.float32) * 0.1).to(bf)
    emb = (torch.randn(B, 2 * nf, 1350, 3072, generator=g, device=device, dtype=torch.float32) * 0.5).to(bf)       # patch-embedded VAE latents, two chunks
    f32 = np.float32
    rope = R.rope_3d_crop(64, (0, 0, 0), (nf, 30, 45), (nf, 30, 45))
    crope = R.rope_3d(64, np.linspace(1000, 1016.25, 5, dtype=f32), np.linspace(0, 30, 8, endpoint=False, dtype=f32), np.linspace(0, 45, 12, endpoint=False, dtype=f32))
    img = R.rope_3d(64, np.arange(13, dtype=f32), np.arange(30, dtype=f32), np.arange(45, dtype=f32))
    smp = R.rope_3d(64, np.linspace(1000, 1013, 4, endpoint=False, dtype=f32), np.linspace(0, 30, 8, endpoint=False, dtype=f32), np.linspace(0, 45, 12, endpoint=False, dtype=f32))
    tgen = torch.Generator().manual_seed(3 + rank)

    def micro():
        ts = torch.randint(0, 1000, (B,), generator=tgen)
        return step.micro_step(x0, noise, ts, text, None, rope, rope, crope, image_embeddings=emb, emb_start_idx=[1, 2], resampler_ropes=(img, smp))

    def fence():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier(); torch.cuda.synchronize()
    for _ in range(a.warmup):
        micro()
    step.micro = 0                                    # the timed region starts at the beginning of an accumulation window
    K.PROFILE_ON[0] = True
    K.PROFILE_FILTER[0] = None if os.environ.get("TG_BENCH_PROFILE_ALL") == "1" else {"attention_bwd"}     # 1: every launch timed (per-shape table, slower step)
    fence()
    power = PowerSampler(device.index or 0)
    with power:
        t0 = time.perf_counter()
        n_opt = 0
        for _ in range(a.steps):
            loss, did = micro()
            n_opt += int(did)
        fence()
        dt = time.perf_counter() - t0
    K.PROFILE_ON[0] = False
    power = power.summary()
    rank_ms = 1e3 * dt / a.steps
    if dist is not None:
        tm = torch.tensor([dt], device=device, dtype=torch.float64)
        dist.all_reduce(tm, op=dist.ReduceOp.MAX)
        dt = float(tm.item())
    # second leg, the yaml's own schedule (cogvideo_5b_vaevip_4x8x12_to2v.yaml:59 gradient_checkpointing: true -> train_cogvideo_to2v.py:1323-1324): every block keeps only
    # its input and re-runs its forward inside the backward (activation_budget_bytes = 0).  Same objects, 1 warm-up + `ckpt_leg_steps` micro-steps from the start of a
    # window (no optimizer step inside unless ckpt_leg_steps >= accum); peak memory counted from a reset
    ckpt_leg = None
    peak_kept = torch.cuda.max_memory_allocated() / 2 ** 30
    kept_blocks = tr.blocks_kept
    if ckpt_leg_steps > 0:
        step.discard_window()
        tr.activation_budget_bytes = 0
        tr._kept, tr._ckpt = {}, []
        for blk in tr._blocks or []:
            blk.saved = None
        import gc
        gc.collect(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
        micro(); step.discard_window()
        fence()
        t0 = time.perf_counter()
        for _ in range(ckpt_leg_steps):
            lc, _ = micro()
        fence()
        cdt = time.perf_counter() - t0
        step.discard_window()
        ckpt_leg = {"schedule": "gradient_checkpointing: true (the yaml's): every block recomputed in the backward", "steps": ckpt_leg_steps, "warmup": 1,
                    "ms_per_step": 1e3 * cdt / ckpt_leg_steps, "blocks_keeping_activations": tr.blocks_kept, "blocks_recomputed_in_backward": a.layers - tr.blocks_kept,
                    "peak_mem_GB": torch.cuda.max_memory_allocated() / 2 ** 30, "loss": float(lc),
                    "step_mfma_frac": TRAIN_FLOP_PER_MICRO_STEP * (a.layers / 42.0) / (cdt / ckpt_leg_steps) / PEAK_BF16,
                    "executed_mfma_frac_incl_recompute": (TRAIN_FLOP_PER_MICRO_STEP + FLOP_PER_STEP) * (a.layers / 42.0) / (cdt / ckpt_leg_steps) / PEAK_BF16}
        tr.activation_budget_bytes = None
    if rank == 0:
        prof = K.profile_summary().get("attention_bwd", {"ms": float("nan"), "n": 0, "total_ms": 0.0})
        # dominant kernel group: the attention backward launches (statistics + dK/dV + dQ).  Algorithmic flops per transformer layer and micro-step:
        # 5 GEMMs (S, dP, dV, dK, dQ) of 2 * nq * nk * 64 per head for the three calls of the processor.
        n1, nv = 226 + 17550, 480
        alg = 5 * 2.0 * 64 * 48 * B * (n1 * n1 + n1 * nv + nv * (n1 + nv)) * a.layers
        tot_ms = prof["total_ms"] / max(1, a.steps)
        traffic = None          # L2-miss bytes of one 17776^2 backward call (dK/dV + dQ launches), from the committed rocprofv3 PMC passes (tools/profile_attn_bwd.sh)
        try:
            with open(os.path.join(ROOT, "profiles", BWD_PMC_SUMMARY)) as f:
                pm = json.load(f)
            traffic = sum(v["l2_miss_traffic_bytes_per_launch"] for k, v in pm.items() if any(t in k for t in ("attn_bwd_dkdv", "attn_bwd_dq", "attn_bwd_fused"))) or None
        except (OSError, KeyError, ValueError):
            pass
        return ({
            "metric": "To2V training samples/sec (micro-steps of per_gpu_batch_size 2, gradient accumulation, clip + AdamW), CogVideoX-5B + Resampler",
            "value": B * world * a.steps / dt, "unit": "samples/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": 1e3 * dt / a.steps,
            "rank_ms_per_step": rank_ms, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16",
            "data": "synthetic latents / embeddings, random-init weights at CogVideoX-5B + Resampler(4x8x12) shapes",
            "config": {"workload": "To2V train micro-step (BASELINE config 5): batch 2 x 13 latent frames 60x90, 226 text + 480 vip tokens, Resampler over 2 chunks of 17550 tokens",
                       "layers": a.layers, "accumulation_steps": a.accum, "optimizer_steps_in_timed_region": n_opt,
                       "blocks_keeping_activations": kept_blocks, "blocks_recomputed_in_backward": a.layers - kept_blocks,
                       "trainable_parameters": int(sum(v.numel() for v in arena.views.values()))},
            # whole micro-step against the MFMA peak: ALGORITHMIC flops of the transformer (forward 776.0 T + attention backward 860.0 T + dgrad through the frozen and vip linears
            # 431.8 T + wgrad of the trainable vip_to_{q,k,v} 86.8 T = 2154.6 T at B = 2; the Resampler's ~1.5 % and any recomputed forward are NOT counted) / time / 2.5 PF
            "step_mfma_frac": TRAIN_FLOP_PER_MICRO_STEP * (a.layers / 42.0) / (dt / a.steps) / PEAK_BF16,
            "flop_per_micro_step": TRAIN_FLOP_PER_MICRO_STEP * (a.layers / 42.0),
            "checkpointed_leg": ckpt_leg,
            "roofline": {"bound": "mfma", "kernel": "tg_attention_bwd (statistics + the one-kernel dK/dV/dQ launch for the 17776^2 and the vip-key calls, dK/dV + dQ launches for the vip-query call; all transformer layers of one micro-step)",
                         "achieved": alg / (tot_ms * 1e-3) / 1e12 if tot_ms > 0 else None, "peak": 2500.0, "unit": "TFLOP/s",
                         "frac": (alg / (tot_ms * 1e-3) / 1e12 / 2500.0) if tot_ms > 0 else None, "traffic": traffic,
                         "traffic_note": "bytes past L2 of ONE main (17776 x 17776, 96 heads) call's backward launch(es) behind the statistics; algorithmic 3.06e9; the one-kernel form's ordered dQ accumulation is 60 GB of L2 read-modify-write, part of which reaches memory",
                         "ms_per_micro_step_in_this_kernel": tot_ms, "launches_per_micro_step": prof["n"] / max(1, a.steps),
                         "frac_at_measured_clock": (alg / (tot_ms * 1e-3) / 1e12 / (2500.0 * power["sclk_MHz_mean"] / 2400.0)) if tot_ms > 0 and power["sclk_MHz_mean"] else None},
            **({"kernel_ms_per_micro_step": {k: round(v["total_ms"] / a.steps, 3) for k, v in sorted(K.profile_summary().items(), key=lambda kv: -kv[1]["total_ms"])},
                "launches_per_micro_step": {k: v["n"] / a.steps for k, v in K.profile_summary().items()}} if K.PROFILE_FILTER[0] is None else {}),
            "loss": float(loss), "grad_norm_last_step": float(opt.coef[0]) if n_opt else None,
            "attention_bwd_form": "one kernel (dK, dV, dQ; ordered dQ exchange, status word checked every micro-step)" if K.BwdDeviceState.get(device).one_kernel
                                  else "two launches (dK/dV + dQ)",
            "attention_bwd_probe": K.BwdDeviceState.get(device).probe,
            "power_W_mean": power["power_W_mean"], "power_cap_W": power["power_cap_W"], "sclk_MHz_mean": power["sclk_MHz_mean"], "limiter": power["limiter"],
            "peak_mem_GB": peak_kept})
    return None


def _r(v, n=4):
    return round(v, n) if isinstance(v, float) else v


def compact_line(out):
    """The ONE JSON line of the bench contract, short enough (< 4 KB) that a record which keeps only the head and the tail of stdout still holds every number
    (the 13 KB line lost `vae` and `train.ms_per_step` in the driver's copy).  `summary` sits right behind `ms_per_step`; no prose.  The full
    record — every key of earlier rounds — goes to gpurun_out/bench_detail.json (copied to profiles/ by the builder)."""
    g = lambda d, *ks: (g(d.get(ks[0]), *ks[1:]) if len(ks) > 1 else d.get(ks[0])) if isinstance(d, dict) else None
    vae, tr, pw, z = out.get("vae"), out.get("train"), out.get("power") or {}, out.get("zero_operand_control")
    ck = g(tr, "checkpointed_leg")
    summary = {"step_mfma_frac": out.get("step_mfma_frac"), "attn_frac": g(out, "roofline", "frac"), "attn_ms": g(out, "roofline", "launch_ms"),
               "zero_ctl_ms": g(z, "ms_per_step"), "power_W": pw.get("power_W_mean"), "power_cap_W": pw.get("power_cap_W"), "sclk_MHz": pw.get("sclk_MHz_mean"),
               "limiter": g(pw, "limiter", "limiter"),
               "vae_decode_s": g(vae, "decode", "seconds"), "vae_encode_s": g(vae, "encode", "seconds"),
               "vae_decode_frac": g(vae, "decode", "frac_of_peak_algorithmic"), "vae_encode_frac": g(vae, "encode", "frac_of_peak_algorithmic"),
               "train_ms_per_micro_step": g(tr, "ms_per_step"), "train_step_mfma_frac": g(tr, "step_mfma_frac"), "train_bwd_frac": g(tr, "roofline", "frac"),
               "train_peak_mem_GB": g(tr, "peak_mem_GB"), "train_ckpt_ms_per_micro_step": g(ck, "ms_per_step"), "train_ckpt_peak_mem_GB": g(ck, "peak_mem_GB"),
               "train_ckpt_step_mfma_frac": g(ck, "step_mfma_frac")}
    line = {k: out[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step")}
    line["summary"] = {k: _r(v) for k, v in summary.items()}
    line.update({k: out[k] for k in ("higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "value_aggregate", "value_per_gpu", "finite", "step_mfma_frac")})
    rf = out["roofline"]
    line["roofline"] = {k: _r(rf.get(k), 5) for k in ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "launch_ms", "launches_timed", "attn_path", "frac_at_measured_clock")}
    if out.get("cpu_baseline"):
        cb = out["cpu_baseline"]
        line["cpu_baseline"] = {k: _r(cb.get(k), 6) for k in ("value", "unit", "cores", "kind", "sample", "fp32_value", "cpu_model", "physical_cores")}
    line["power"] = {"W_mean": _r(pw.get("power_W_mean"), 1), "cap_W": pw.get("power_cap_W"), "sclk_MHz_mean": _r(pw.get("sclk_MHz_mean"), 1), "limiter": pw.get("limiter")}
    if z:
        line["zero_operand_control"] = {"ms_per_step": _r(z["ms_per_step"], 2), "attention_launch_ms": _r(z["attention_launch_ms"], 3), "W_mean": _r(z.get("power_W_mean"), 1),
                                        "sclk_MHz_mean": _r(z.get("sclk_MHz_mean"), 1), "limiter": g(z, "limiter", "limiter")}
    km = sorted(out.get("kernel_ms", {}).items(), key=lambda kv: -kv[1])[:6]
    line["kernel_ms_top"] = {k: _r(v, 3) for k, v in km}
    line["rank_ms_per_step"] = out.get("rank_ms_per_step")
    if vae:
        line["vae"] = {n: {"seconds": _r(vae[n]["seconds"]), "frac_algorithmic": _r(vae[n]["frac_of_peak_algorithmic"]), "frac_executed": _r(vae[n]["frac_of_peak_executed"]),
                           "W_mean": _r(vae[n]["power_W_mean"], 1), "sclk_MHz_mean": _r(vae[n]["sclk_MHz_mean"], 1),
                           "ppt_active_frac": g(vae[n], "limiter", "active_frac", "ppt")} for n in ("decode", "encode")}
    if tr:
        line["train"] = {"value": _r(tr["value"]), "unit": tr["unit"], "steps": tr["steps"], "ms_per_step": _r(tr["ms_per_step"], 2), "step_mfma_frac": _r(tr["step_mfma_frac"]),
                         "flop_per_micro_step": tr["flop_per_micro_step"], "optimizer_steps_in_timed_region": g(tr, "config", "optimizer_steps_in_timed_region"),
                         "blocks_recomputed_in_backward": g(tr, "config", "blocks_recomputed_in_backward"), "peak_mem_GB": _r(tr["peak_mem_GB"], 2),
                         "roofline": {k: _r(g(tr, "roofline", k), 5) for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "ms_per_micro_step_in_this_kernel")},
                         "loss": _r(tr["loss"], 5), "grad_norm_last_step": _r(tr["grad_norm_last_step"], 4), "W_mean": _r(tr["power_W_mean"], 1), "sclk_MHz_mean": _r(tr["sclk_MHz_mean"], 1),
                         "checkpointed_leg": None if not ck else {k: _r(ck[k]) for k in ("steps", "ms_per_step", "blocks_recomputed_in_backward", "peak_mem_GB", "step_mfma_frac",
                                                                                         "executed_mfma_frac_incl_recompute")}}
    line["detail"] = "gpurun_out/bench_detail.json"
    return line


def emit(out):
    """Full record to the scratch file gpurun_out/bench_detail.json (nothing long on stdout or stderr: a record that keeps head and tail of the streams must keep the
    contract line whole), then the compact contract line as the only line of stdout."""
    detail = json.dumps(out)
    try:
        os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
        with open(os.path.join(ROOT, "gpurun_out", "bench_detail.json"), "w") as f:
            f.write(detail + "\n")
    except OSError:
        pass
    print(json.dumps(compact_line(out)))
    sys.stdout.flush()


def dump_outputs(d, arrays):
    """`arrays` (name -> device tensor, what a caller of the timed path receives) as float32 `d/<name>.npy`: the files two builds are compared on."""
    os.makedirs(d, exist_ok=True)
    for name, t in arrays.items():
        np.save(os.path.join(d, name + ".npy"), t.float().cpu().numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--layers", type=int, default=42, help="debug only: anything but 42 is not the benchmark")
    ap.add_argument("--mode", choices=("window", "e2e", "gen", "train"), default="window",
                    help="window (default, the headline): steady-state FIFO window steps; e2e: one whole To2V run incl. ramp, base stage, VAE decode; "
                         "gen: e2e preceded by the T2To token stage (gen.yaml, BASELINE config 3); train: To2V training micro-steps (BASELINE config 5)")
    ap.add_argument("--accum", type=int, default=9, help="--mode train: gradient_accumulation_steps (yaml: 9)")
    ap.add_argument("--chunks", type=int, default=12, help="--mode e2e: number of 49-frame clips (edit.yaml: 12)")
    ap.add_argument("--full", action="store_true",
                    help="window mode: besides the headline, the full record — attention launches timed with HIP events, the other attention path, power and clock, "
                         "zero-operand control, VAE and training sub-records, CPU baseline — written to the detail file; without it only setup, warm-up, the timed steps "
                         "and the result line")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="window mode: write what the last timed step returned (window latents and x0) to DIR/<name>.npy as float32")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--no-vae", action="store_true", help="--full: skip the VAE (BASELINE config 4) sub-record")
    ap.add_argument("--no-train", action="store_true", help="--full: skip the training (BASELINE config 5) sub-record")
    ap.add_argument("--no-zero-control", action="store_true", help="--full: skip the zero-operand control (3 untimed steps on zeroed weights and inputs)")
    a = ap.parse_args()
    if a.steps < 1:
        ap.error("--steps must be at least 1")
    if a.dump_outputs and a.mode != "window":
        ap.error("--dump-outputs applies to --mode window")

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the hot path has no CPU fallback")
    if a.gpus > 1 and "RANK" not in os.environ:
        # not under torch.distributed.run: start the N ranks ourselves (one process per GPU, RCCL) and supervise them
        if torch.cuda.device_count() < a.gpus:
            raise SystemExit(f"bench.py --gpus {a.gpus}: only {torch.cuda.device_count()} GPU(s) visible")
        from tokensgen_amd.runtime import launch
        launch(a.gpus, [sys.executable, os.path.abspath(__file__)] + sys.argv[1:])
        return
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    dist = None
    use_dist = "RANK" in os.environ            # launched by torch.distributed.run or by the branch above (also exercised with 1 rank)
    if use_dist:
        import torch.distributed as dist
        from tokensgen_amd.runtime import init_distributed
        init_distributed("nccl", device=device)

    from tokensgen_amd import kernels as K
    from tokensgen_amd import lib
    from tokensgen_amd.fifo import FifoWorker
    from tokensgen_amd.scheduler import CogVideoXDPMScheduler
    from tokensgen_amd import rope as R
    lib.load()
    if a.mode in ("e2e", "gen", "train"):
        (run_train if a.mode == "train" else run_e2e)(a, rank, world, device, dist)
        if use_dist:
            dist.destroy_process_group()
        return

    model = build_model(device, a.layers)
    sched = CogVideoXDPMScheduler(prediction_type="v_prediction", rescale_betas_zero_snr=True, snr_shift_scale=1.0,
                                  timestep_spacing="trailing")
    sched.set_timesteps(52)
    g = torch.Generator(device=device).manual_seed(42 + rank)
    nf, C, H, W = 13, 16, 60, 90
    bf = torch.bfloat16
    latents = torch.randn(1, nf, C, H, W, generator=g, device=device, dtype=torch.float32).to(bf)
    old_x0 = torch.randn(nf, C, H, W, generator=g, device=device, dtype=torch.float32).to(bf)
    prompt = (torch.randn(2, 226, 4096, generator=g, device=device, dtype=torch.float32) * 0.1).to(bf)
    emb = torch.nn.functional.layer_norm(torch.randn(1, 5, 8, 12, 3072, generator=g, device=device), (3072,))
    emb = emb.permute(0, 1, 4, 2, 3).to(bf).repeat(2, 1, 1, 1, 1).contiguous()
    f32 = np.float32
    rope = R.rope_3d_crop(64, (0, 0, 0), (nf, 30, 45), (nf, 30, 45))
    worker = FifoWorker(model, sched, prompt, rope, 6.0, np.arange(30, dtype=f32), np.arange(45, dtype=f32),
                        np.linspace(0, 30, 8, endpoint=False, dtype=f32), np.linspace(0, 45, 12, endpoint=False, dtype=f32))
    ts = sched.timesteps.tolist()
    # a steady-state window: rank r of 8 covers queue positions [13*(r//2)+6*(r%2), +13)  
    r8 = rank % 8
    start = 13 * (r8 // 2) + 6 * (r8 % 2)
    lvl = ([18] * 6 + ts[::-1])
    t = lvl[start:start + nf]
    prev_t = [(-1 if q <= 6 else lvl[q - 1]) for q in range(start, start + nf)]
    next_t = [(lvl[q + 1] if q + 1 < len(lvl) else -1) for q in range(start, start + nf)]
    has_old = [nt > 0 for nt in next_t]
    grid_t = np.arange(nf, dtype=f32) + f32(start)
    cond_t = np.linspace(1000, 1016.25, 5, dtype=f32)
    # the exchange of tokensgen_amd/fifo.py:226-243, one window per rank: [x | x0] of the whole window + 8 elements carrying the failure flag
    n_el = 2 * nf * C * H * W
    xbuf = torch.zeros(n_el + 8, device=device, dtype=bf)
    gathered = torch.empty(world * (n_el + 8), device=device, dtype=bf) if use_dist else None   # rank-major concat

    def step():
        noise = torch.randn(nf, 2, C, H, W, generator=g, device=device, dtype=torch.float32).to(bf)
        x, x0 = worker.window_step(latents, old_x0, has_old, t, prev_t, next_t, noise, grid_t, cond_t, emb)
        if use_dist:
            buf = xbuf[:n_el].view(2, nf, C, H, W)
            buf[0], buf[1] = x[0], x0
            dist.all_gather_into_tensor(gathered, xbuf)
        return x, x0

    def fence():
        torch.cuda.synchronize()
        if use_dist:
            dist.barrier()
            torch.cuda.synchronize()

    for _ in range(a.warmup):
        step()
    fence()
    ATTN = "attention_2seg+rider"
    if a.full:
        # inside the timed region only the dominant kernel's launches are bracketed by HIP events (on the launch stream); the other
        # kernels' durations come from one extra, untimed step afterwards, so their ~1800 event markers do not sit in the measurement
        K.PROFILE.clear(); K.PROFILE_FILTER[0] = {ATTN}; K.PROFILE_ON[0] = True
    # --full: a host thread reading sysfs / amdsmi: no GPU work, nothing on the launch stream
    power = PowerSampler(local_rank) if a.full else contextlib.nullcontext()
    with power:
        t0 = time.perf_counter()
        for _ in range(a.steps):
            x_last, x0_last = step()
        fence()
        dt = time.perf_counter() - t0
    attn_path = model.attn_path                      # what the timed region ran on ("constant_shift" unless the retry counter said otherwise)
    finite = bool(torch.isfinite(x_last).all())
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, {"latents": x_last, "x0": x0_last})
    if a.full:
        K.PROFILE_ON[0] = False
        power = power.summary()
        attn_prof = K.profile_summary().get(ATTN, {"ms": float("nan"), "n": 0})
        retry_ws = next(iter(model._ws.values())).retry
        retried = retry_ws.count()
        K.PROFILE.clear(); K.PROFILE_FILTER[0] = None; K.PROFILE_ON[0] = True
        step()
        fence()
        K.PROFILE_ON[0] = False
        all_prof = K.profile_summary()
        # the other attention path, one untimed step, so that the headline's dependence on the path is on the record
        other = "running_max" if attn_path == "constant_shift" else "constant_shift"
        model.attn_path = other
        K.PROFILE.clear(); K.PROFILE_FILTER[0] = {ATTN}; K.PROFILE_ON[0] = True
        t1 = time.perf_counter()
        step()
        fence()
        other_step_ms = 1e3 * (time.perf_counter() - t1)
        K.PROFILE_ON[0] = False
        other_prof = K.profile_summary().get(ATTN, {"ms": float("nan"), "n": 0})
        model.attn_path = attn_path
        # zero-operand control (untimed, rank-local, AFTER everything that needs the weights): the same launches on all-zero weights and inputs.  With nothing
        # toggling in the matrix pipe the chip is no longer on its socket power cap; the ratio to `ms_per_step` is how much of the headline is clock, not schedule
        zero_ctl = None
        if world == 1 and not a.no_zero_control:
            keep = {k: t.clone() for k, t in model._fused.items()}
            for t_ in model._fused.values():
                t_.zero_()
            zl, zx0, zp, ze = latents.clone(), old_x0.clone(), prompt.clone(), emb.clone()
            latents.zero_(); old_x0.zero_(); prompt.zero_(); emb.zero_()
            znoise = torch.zeros(nf, 2, C, H, W, device=device, dtype=bf)

            def zstep():
                return worker.window_step(latents, old_x0, has_old, t, prev_t, next_t, znoise, grid_t, cond_t, emb)
            zstep(); fence()
            K.PROFILE.clear(); K.PROFILE_FILTER[0] = {ATTN}; K.PROFILE_ON[0] = True
            zpow = PowerSampler(local_rank)
            with zpow:
                t1 = time.perf_counter()
                for _ in range(3):
                    zx = zstep()
                fence()
                zdt = time.perf_counter() - t1
            K.PROFILE_ON[0] = False
            zattn = K.profile_summary().get(ATTN, {"ms": float("nan"), "n": 0})
            zero_ctl = {"what": "the same 3 window steps with every weight and every input zeroed (same launches, same schedules; timing only)", "steps": 3,
                        "ms_per_step": 1e3 * zdt / 3, "attention_launch_ms": zattn["ms"], "finite": bool(torch.isfinite(zx[0]).all()), **zpow.summary()}
            for k, t_ in model._fused.items():
                t_.copy_(keep[k])
            latents.copy_(zl); old_x0.copy_(zx0); prompt.copy_(zp); emb.copy_(ze)
            del keep, zl, zx0, zp, ze
    rank_ms = [1e3 * dt / a.steps]
    if use_dist:
        mine = torch.tensor([dt], device=device, dtype=torch.float64)
        every = torch.empty(world, device=device, dtype=torch.float64)
        dist.all_gather_into_tensor(every, mine)
        rank_ms = [1e3 * v / a.steps for v in every.tolist()]
        dt = float(every.max().item())
    if rank == 0:
        # the headline: all a plain run computes and prints
        line = {
            "metric": "DiT denoising steps/sec, CogVideoX-5B To2V 720x480 (CFG-batched 13-frame FIFO window: DiT fwd + CFG + 13 DPM updates)",
            # `value` is the WHOLE-JOB aggregate over the N ranks (the bench contract); BASELINE's metric is quoted per GPU: that is value_per_gpu.
            # At N = 1 the two coincide.  Each rank runs a steady-state window (weak scaling); the end-to-end rate incl. the ramp is `--mode e2e`.
            "value": world * a.steps / dt, "unit": "steps/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": 1e3 * dt / a.steps, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "bf16", "data": "synthetic latents/embeddings, random-init weights at CogVideoX-5B shapes",
            "config": {"workload": "To2V FIFO window step, CogVideoX-5B 42 layers D=3072, 226 text + 17550 video + 480 vip tokens, CFG batch 2, DPM-solver++",
                       "layers": a.layers, "exchange": "RCCL all_gather of kept half-windows per step" if use_dist else "none"},
            "value_aggregate": world * a.steps / dt, "value_per_gpu": a.steps / dt, "finite": finite,
            "step_mfma_frac": FLOP_PER_STEP * (a.layers / 42.0) * (a.steps / dt) / PEAK_BF16,
            "rank_ms_per_step": [round(v, 3) for v in rank_ms], "attn_path": attn_path,
        }
        if not a.full:
            print(json.dumps(line))
            sys.stdout.flush()
    if rank == 0 and a.full:
        prof = all_prof
        attn = attn_prof
        attn_s = attn["ms"] * 1e-3
        achieved = ATTN_FLOP_PER_LAUNCH / attn_s / 1e12 if attn["n"] else float("nan")
        traffic = None          # HBM-side bytes per launch of the dominant kernel, from the committed rocprofv3 PMC passes
        try:
            with open(os.path.join(ROOT, "profiles", PMC_SUMMARY)) as f:
                traffic = json.load(f)["_derived"]["attention_main_traffic_bytes_per_launch"]
        except (OSError, KeyError, ValueError):
            pass
        out = dict(line, **{
            "value_is": "aggregate over n_gpus",
            "leg": "steady_state (one full window per rank per step; end to end incl. ramp / base stage / decode: --mode e2e, strong scaling)",
            "roofline": {"bound": "mfma", "kernel": "attn_fwd_pp_kernel (tg_attention_fwd_multi: SDPA#1+#2 fused, SDPA#3 riding, key-split tail + combine)", "achieved": achieved,
                         "peak": PEAK_BF16 / 1e12, "unit": "TFLOP/s", "frac": achieved / (PEAK_BF16 / 1e12), "traffic": traffic,
                         "launch_ms": attn["ms"], "launches_timed": attn["n"], "attn_path": attn_path},
            "attn_retried_workgroups": retried,
            "roofline_other_attn_path": {"attn_path": other, "launch_ms": other_prof["ms"], "launches_timed": other_prof["n"],
                                         "achieved": ATTN_FLOP_PER_LAUNCH / (other_prof["ms"] * 1e-3) / 1e12,
                                         "frac": ATTN_FLOP_PER_LAUNCH / (other_prof["ms"] * 1e-3) / PEAK_BF16, "step_ms_one_untimed_step": other_step_ms},
            "kernel_ms": {k: round(v["ms"], 4) for k, v in prof.items()},
            # socket power and shader clock over the timed region (PowerSampler), top level so that the driver's record carries them
            "power_W_mean": power["power_W_mean"], "power_cap_W": power["power_cap_W"], "sclk_MHz_mean": power["sclk_MHz_mean"], "power": power,
            "zero_operand_control": zero_ctl,
        })
        sclk = power["sclk_MHz_mean"]
        # the same achieved rates against the peak AT THE CLOCK THE CHIP ACTUALLY RAN (2.5 PF is quoted at 2400 MHz)
        out["roofline"]["frac_at_measured_clock"] = achieved / (PEAK_BF16 / 1e12 * sclk / 2400.0) if sclk else None
        out["step_mfma_frac_at_measured_clock"] = out["step_mfma_frac"] / (sclk / 2400.0) if sclk else None
        if not a.no_vae and world == 1:
            out["vae"] = vae_record(device)
        if not a.no_train and world == 1 and a.layers == 42:
            # BASELINE config 5 on the driver's record (outside the timed region, like `vae`): the inference model is released first
            worker = model = retry_ws = None          # (the step closure sees the same cells: nothing keeps the 14 GB of weights + workspaces)
            import gc
            gc.collect(); torch.cuda.empty_cache()
            ta = argparse.Namespace(layers=a.layers, steps=9, warmup=1, accum=9)      # one whole accumulation window: the optimizer step is inside
            out["train"] = train_measure(ta, 0, 1, device, None, ckpt_leg_steps=3)
        if not a.no_cpu_baseline and world == 1:
            out["cpu_baseline"] = cpu_baseline()
        emit(out)
    if use_dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
