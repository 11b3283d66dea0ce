"""CPU: host logic of the product (no kernels run): RoPE tables, scheduler tables, packing of the fused weight
storages, and that the C-ABI library exports every symbol include/tokensgen_hip.h declares."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle import dit_ref as O
from oracle import scheduler_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rope_tables_bit_exact_vs_oracle():
    from tokensgen_amd import rope as R
    f32 = np.float32
    for gt, gh, gw in [(np.arange(13, dtype=f32), np.arange(30, dtype=f32), np.arange(45, dtype=f32)),
                       (np.linspace(1000, 1016.25, 5, dtype=f32), np.linspace(0, 30, 8, endpoint=False, dtype=f32),
                        np.linspace(0, 45, 12, endpoint=False, dtype=f32)),
                       (np.arange(13, dtype=f32) + f32(137.0), np.arange(4, dtype=f32), np.arange(6, dtype=f32))]:
        a, b = R.rope_3d(64, gt, gh, gw), O.rope_3d(64, gt, gh, gw)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    a, b = R.rope_3d_crop(64, (0, 0, 0), (13, 30, 45), (13, 30, 45)), O.rope_3d_crop(64, (0, 0, 0), (13, 30, 45), (13, 30, 45))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # T2To split 52/6/6 (pipeline_cogvideox_t2to.py:557-559)
    a = R.rope_3d(64, np.arange(4, dtype=f32), np.arange(8, dtype=f32), np.arange(12, dtype=f32), 52, 6, 6)
    b = O.rope_3d(64, np.arange(4, dtype=f32), np.arange(8, dtype=f32), np.arange(12, dtype=f32), 52, 6, 6)
    assert torch.equal(a[0], b[0]) and a[0].shape == (384, 64)


def test_scheduler_tables_vs_oracle(golden_dir):
    from tokensgen_amd.scheduler import CogVideoXDPMScheduler, dpm_coef_row
    s = CogVideoXDPMScheduler(prediction_type="v_prediction", rescale_betas_zero_snr=True, snr_shift_scale=1.0,
                              timestep_spacing="trailing")
    s.set_timesteps(52)
    g = torch.load(os.path.join(golden_dir, "scheduler.pt"), weights_only=False)
    assert torch.equal(s.timesteps, g["timesteps"])
    assert (s.alphas_cumprod - g["alphas_cumprod"]).abs().max() < 1e-15 and s.alphas_cumprod[-1] == 0
    assert torch.equal(s.betas, g["betas"])
    _, ac = S.alphas_cumprod()
    ts = s.timesteps.tolist()
    for i in range(1, 51):
        row = dpm_coef_row(s.alphas_cumprod.numpy(), ts[i], ts[i + 1], ts[i - 1], True)
        c = S.step_coefficients(ac, ts[i], ts[i + 1], ts[i - 1])
        ref = [float(c[k]) for k in ("sa", "sb", "m1", "m2", "m3", "m4", "mn")]
        assert np.allclose(row[:7], ref, rtol=1e-12, atol=1e-14) and row[7] == 1.0
    # edges: t=999 first step (no x0 yet), prev_t=-1 final step
    assert dpm_coef_row(s.alphas_cumprod.numpy(), 999, 980, None, False)[2] == 0.0
    last = dpm_coef_row(s.alphas_cumprod.numpy(), 18, -1, 37, True)
    assert last[2] == 0.0 and last[3] == -1.0 and last[6] == 0.0 and last[7] == 0.0
    with pytest.raises(NotImplementedError):
        CogVideoXDPMScheduler(beta_schedule="vip_1")
    for sp, n in (("leading", 50), ("linspace", 7)):
        CogVideoXDPMScheduler(prediction_type="v_prediction", timestep_spacing=sp).set_timesteps(n)


def test_transformer_state_dict_contract():
    """Reference key names, fused storages shared with the named parameters, vip layers added later."""
    from tokensgen_amd.transformer import CogVideoXTransformer3DModel, VideoIPAdapterCogVideoXAttnProcessor2_0
    cfg = dict(num_attention_heads=2, attention_head_dim=64, num_layers=2, patch_size=2, time_embed_dim=128,
               text_embed_dim=64, in_channels=16, out_channels=16)
    m = CogVideoXTransformer3DModel(num_attention_heads=2, attention_head_dim=64, num_layers=2, time_embed_dim=128,
                                    text_embed_dim=64, use_rotary_positional_embeddings=True, device="cpu")
    assert sorted(m.state_dict()) == sorted(O.make_state_dict(cfg, None, seed=1))
    base = {k: v.to(torch.bfloat16) for k, v in O.make_state_dict(cfg, None, seed=1).items()}
    m.load_state_dict(base, strict=True)
    vipcfg = dict(length=30, func_type="1", scale=[0.6],
                  resampler_params=dict(output_dim=128, num_height_queries=2, num_width_queries=3, num_temporal_queries=4))
    m.set_vip_layers(None, **vipcfg)
    sd = {k: v.to(torch.bfloat16) for k, v in O.make_state_dict(cfg, 128, seed=1).items()}
    assert sorted(m.state_dict()) == sorted(sd)
    # set_vip_layers initialises the vip projections from the base ones (cogvideox_transformer_3d.py:207-218)
    assert torch.equal(m.state_dict()["transformer_blocks.1.attn1.processor.vip_to_k.weight"], base["transformer_blocks.1.attn1.to_k.weight"])
    # ... and keeps the already-loaded modulation weights when the fused matrix is re-laid-out
    assert torch.equal(m.state_dict()["transformer_blocks.1.norm2.linear.weight"], base["transformer_blocks.1.norm2.linear.weight"])
    m.load_state_dict(sd, strict=True)
    D = 128
    per, out_base, total = m._mod_cols()
    assert (per, out_base, total) == (18 * D, 36 * D, 38 * D)
    assert torch.equal(m._fused["mod.w"][per + 9 * D: per + 15 * D], sd["transformer_blocks.1.norm2.linear.weight"])
    assert torch.equal(m._fused["mod.w"][per + 6 * D: per + 9 * D], sd["transformer_blocks.1.vip_norm1.linear.weight"])
    assert torch.equal(m._fused["l0.vqkv.w"][2 * D:], sd["transformer_blocks.0.attn1.processor.vip_to_v.weight"])
    assert torch.equal(m._fused["patch.w"], sd["patch_embed.proj.weight"].reshape(D, 64))
    assert m._fused["proj_out.w"].shape == (128, D) and (m._fused["proj_out.w"][64:] == 0).all()
    procs = [mod for mod in m.modules() if mod.__class__.__name__ == "VideoIPAdapterCogVideoXAttnProcessor2_0"]
    assert len(procs) == 2 and isinstance(procs[0], VideoIPAdapterCogVideoXAttnProcessor2_0) and procs[0].scale == [0.6]
    # vip.pt round trip (save_vip_layers / set_vip_layers(vip_ckpt_dir), cogvideox_transformer_3d.py:603-634)
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        m.save_vip_layers(d)
        saved = torch.load(os.path.join(d, "vip.pt"), weights_only=True)
        assert all("vip_" in k for k in saved) and len(saved) == 2 * 18 + 2
        m2 = CogVideoXTransformer3DModel(num_attention_heads=2, attention_head_dim=64, num_layers=2, time_embed_dim=128,
                                         text_embed_dim=64, use_rotary_positional_embeddings=True, device="cpu")
        m2.load_state_dict(base, strict=True)
        m2.set_vip_layers(d, **vipcfg)
        sd2 = m2.state_dict()
        assert all(torch.equal(sd2[k].float(), v) for k, v in saved.items())
        assert torch.equal(m2._fused["l1.vqkv.w"], m._fused["l1.vqkv.w"])
        assert torch.equal(sd2["transformer_blocks.0.norm1.linear.weight"], base["transformer_blocks.0.norm1.linear.weight"])
        with pytest.raises(IOError):
            m2.set_vip_layers(os.path.join(d, "missing"), **vipcfg) if os.makedirs(os.path.join(d, "missing")) is None else None


def test_no_cpu_fallback():
    """The product path must fail loudly without a GPU — never route through torch/CPU."""
    from tokensgen_amd.transformer import CogVideoXTransformer3DModel
    m = CogVideoXTransformer3DModel(num_attention_heads=2, attention_head_dim=64, num_layers=1, time_embed_dim=128,
                                    text_embed_dim=64, use_rotary_positional_embeddings=True, device="cpu")
    z = torch.zeros
    with pytest.raises(RuntimeError, match="GPU"):
        m(z(1, 13, 16, 4, 6, dtype=torch.bfloat16), z(1, 8, 64, dtype=torch.bfloat16), z(1, dtype=torch.long),
          image_rotary_emb=(z(78, 64), z(78, 64)))
    with pytest.raises(NotImplementedError):
        CogVideoXTransformer3DModel(num_attention_heads=2, attention_head_dim=32, use_rotary_positional_embeddings=True, device="cpu")


def test_c_abi_exports_every_declared_symbol():
    from tokensgen_amd import lib as L
    hdr = open(os.path.join(ROOT, "include", "tokensgen_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(tg_[a-z0-9_]+)\s*\(", hdr))
    assert {"tg_gemm_bf16", "tg_attention_fwd", "tg_adaln_modulate", "tg_qk_layernorm_rope", "tg_cfg_dpm_step"} <= declared
    assert os.path.exists(L.LIB_PATH), "build the library first: python -c 'import __graft_entry__ as g; g.build()'"
    so = ctypes.CDLL(L.LIB_PATH)
    for name in declared:
        assert hasattr(so, name), f"{name} declared in include/tokensgen_hip.h but not exported"
    lib = L.load()
    assert set(L.PROTOTYPES) | set(L.QUERIES) | set(L.OTHER_EXPORTS) == declared
    assert b"gfx950" in lib.tg_version()
    # ... and NOTHING ELSE: the library is built with -fvisibility=hidden, `nm -D` of its defined symbols == the header's declarations
    import subprocess
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if len(ln.split()) >= 3 and ln.split()[-2] in "TWBDRV"}
    exported -= {"_init", "_fini", "__bss_start", "_edata", "_end"}
    exported = {n for n in exported if not n.startswith("__hip_")}          # the HIP fat-binary registration objects of every hipcc-built library
    assert exported == declared, (sorted(exported - declared), sorted(declared - exported))
    # the product sources read no environment variable, and the test-only cross-check kernels are not in the product library
    csrc = os.path.join(ROOT, "tokensgen_amd", "csrc")
    for f in os.listdir(csrc):
        if f.endswith((".hip", ".cpp", ".h")):
            assert "getenv" not in open(os.path.join(csrc, f)).read(), f
    assert not os.path.exists(os.path.join(csrc, "attention_bwd_ref.hip"))
    # the debug knobs: defaults, set / get round trip, unknown names refused
    val = ctypes.c_long(-1)
    assert lib.tg_debug_get(b"TG_ATTN_PP_MIN_WG", ctypes.byref(val)) == 0 and val.value == 1024
    assert L.debug_set("TG_GEMM_W4", 0) == 1 and L.debug_set("TG_GEMM_W4", 1) == 0
    assert lib.tg_debug_set(b"TG_NO_SUCH_KNOB", 1) == -1 and b"unknown knob" in lib.tg_last_error_string()
    names = []
    while lib.tg_debug_knob_name(len(names)) is not None:
        names.append(lib.tg_debug_knob_name(len(names)).decode())
    assert names == ["TG_ATTN_PP_MIN_WG", "TG_ATTN_FIXEDM", "TG_ATTN_SPLIT", "TG_GEMM_W4", "TG_CONV_SPLITK", "TG_CONV_HALO", "TG_CONV_W4"]
    # argument validation happens before any launch, so it is testable without a GPU
    assert lib.tg_gemm_bf16(None, 0, 0, None, 0, None, None, 0, 0, 1, 128, 64, 1, 0, None, 0, 0, None, None) == -1
    assert b"null pointer" in lib.tg_last_error_string()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf) + (16 - ctypes.addressof(buf) % 16)
    assert lib.tg_gemm_bf16(p, 64, 0, p, 64, None, p, 100, 0, 4, 100, 64, 1, 0, None, 0, 0, None, None) == -2
    assert b"N%128" in lib.tg_last_error_string()
    # the epilogue enum of the header == the constants of the binding; the two training-step epilogues refuse shapes without the 4-wave kernel (no launch: testable here)
    raw = open(os.path.join(ROOT, "include", "tokensgen_hip.h")).read()
    enum = dict(re.findall(r"\b(TG_EPI_[A-Z_]+)\s*=\s*(\d+)", raw))
    assert {k: int(v) for k, v in enum.items()} == {"TG_EPI_BIAS": L.EPI_BIAS, "TG_EPI_BIAS_GELU": L.EPI_BIAS_GELU, "TG_EPI_BIAS_SILU": L.EPI_BIAS_SILU,
                                                    "TG_EPI_BIAS_GATE_RES": L.EPI_BIAS_GATE_RES, "TG_EPI_BIAS_KEEP_GELU": L.EPI_BIAS_KEEP_GELU,
                                                    "TG_EPI_BIAS_MUL_GELU_GRAD": L.EPI_BIAS_MUL_GELU_GRAD}
    for epi in (L.EPI_BIAS_KEEP_GELU, L.EPI_BIAS_MUL_GELU_GRAD):
        assert lib.tg_gemm_bf16(p, 64, 0, p, 64, None, p, 128, 0, 512, 128, 64, 1, epi, p, 128, 0, None, None) == -2 and b"4-wave kernel only" in lib.tg_last_error_string()
        assert lib.tg_gemm_bf16(p, 64, 0, p, 64, None, p, 128, 0, 512, 128, 64, 1, epi, None, 128, 0, None, None) == -1


def test_c_abi_rejects_null_arguments_everywhere():
    """Error convention of the boundary: EVERY export, called with null pointers and zero sizes, returns a negative code and leaves a
    message in tg_last_error_string() — it validates before it touches HIP, so this holds on a box without a GPU, and nothing crosses the ABI as a
    crash.  Run in a child process so that a missing check would show up as a failed test, not as a dead test session."""
    import subprocess
    import sys
    code = r"""
import ctypes as C, sys
sys.path.insert(0, %r)
from tokensgen_amd import lib as L
lib = L.load()
bad = []
for name, argtypes in L.PROTOTYPES.items():
    if name == "tg_attention_bwd_probe_verdict":      # a predicate (0 / 1), not a launch
        assert lib.tg_attention_bwd_probe_verdict(None, 0) == 0
        continue
    args = [None if (t is C.c_void_p or (isinstance(t, type) and issubclass(t, C._Pointer))) else (0.0 if t is C.c_float else 0) for t in argtypes]
    rc = getattr(lib, name)(*args)
    if not (rc < 0 and lib.tg_last_error_string()):
        bad.append((name, rc))
print("checked", len(L.PROTOTYPES), "bad", bad)
assert not bad
""" % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "bad []" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_longvgen_alias_and_vae_host_contract():
    import sys
    from tokensgen_amd import compat
    from tokensgen_amd.vae import AutoencoderKLCogVideoX
    from oracle import vae_ref as V
    assert "longvgen" not in sys.modules
    compat.install_longvgen_alias()
    try:
        from longvgen.models import CogVideoXTransformer3DModel, AutoencoderKLCogVideoX as A2
        from longvgen.schedulers import CogVideoXDPMScheduler
        from longvgen.fifo_sampling import cogvideo_fifo_mp_v2
        from longvgen.pipeline import MPFIFOVideoIPAdapterCogVideoXPipeline, LongVGenCogVideoXPipeline
        from longvgen.video_ipadapter import Resampler
        assert A2 is AutoencoderKLCogVideoX and callable(cogvideo_fifo_mp_v2) and callable(LongVGenCogVideoXPipeline) and callable(Resampler)
        with pytest.raises(ImportError):
            import longvgen.data  # noqa: F401  (out of scope: never silently stubbed)
    finally:
        for k in [k for k in sys.modules if k == "longvgen" or k.startswith("longvgen.") or k == "pca"]:
            del sys.modules[k]
    vae = AutoencoderKLCogVideoX(device="cpu")
    assert (vae.tile_sample_min_height, vae.tile_sample_min_width, vae.tile_latent_min_height, vae.tile_latent_min_width) == (240, 360, 30, 45)
    assert vae.config.scaling_factor == 1.15258426 and vae._frame_batches(13, 2) == V.frame_batches(13, 2) and vae._frame_batches(49, 8) == V.frame_batches(49, 8)
    cfg = dict(block_out_channels=(64, 128, 128, 128), layers_per_block=1, latent_channels=16, sample_height=64, sample_width=96)
    v2 = AutoencoderKLCogVideoX(block_out_channels=cfg["block_out_channels"], layers_per_block=1, sample_height=64, sample_width=96, device="cpu")
    sd = V.make_state_dict(cfg, seed=1)
    v2.load_state_dict(sd)
    assert sorted(v2.state_dict()) == sorted(sd)
    w = v2._packed["decoder.conv_in.conv.weight"]                 # [Cout_pad, taps, Cin_pad], taps ordered (dt, dh, dw)
    assert w.shape == (128, 27, 64) and torch.equal(w[:128, 5, :16].float(), sd["decoder.conv_in.conv.weight"][:, :, 0, 1, 2].to(torch.bfloat16).float())
    assert (w[:, :, 16:] == 0).all()
    with pytest.raises(RuntimeError, match="GPU"):
        v2.decode(torch.zeros(1, 16, 3, 4, 6))
    with pytest.raises(NotImplementedError):
        AutoencoderKLCogVideoX(latent_channels=8, device="cpu")


def test_pca_holder_matches_reference_fit_and_unpickles_under_the_reference_module_name(golden_dir, tmp_path):
    """tokensgen_amd.pca.PCA: the fit/inverse algebra (pca.py:11-66), and a pickle written under the module name `pca` (what the
    reference's torch.save of its own object produces) loads through the alias — the T2To pipeline torch.load()s such a file."""
    import sys
    from tokensgen_amd import compat
    from tokensgen_amd.pca import PCA
    g = torch.Generator().manual_seed(11)
    X = torch.randn(200, 12, generator=g) * torch.linspace(3, 0.2, 12)
    p = PCA(n_components=5).fit(X)
    assert p.components_.shape == (5, 12) and p.mean_.shape == (1, 12)
    assert torch.allclose(p.components_ @ p.components_.t(), torch.eye(5), atol=1e-5)
    U, Sv, Vt = torch.linalg.svd(X - X.mean(0, keepdim=True), full_matrices=False)
    assert torch.allclose(p.components_.abs(), Vt[:5].abs(), atol=1e-5)
    full = PCA().fit(X)
    assert torch.allclose(full.inverse_transform(full.transform(X)), X, atol=1e-4)
    # the fixture's 16 rows came from the reference class fitted on seeded data: same sign convention (largest |u| positive)
    t = torch.load(os.path.join(golden_dir, "t2to_tiny.pt"), weights_only=False)
    assert t["pca_components16"].shape == (16, 3072) and torch.allclose(t["pca_components16"] @ t["pca_components16"].t(), torch.eye(16), atol=1e-4)
    compat.install_longvgen_alias()
    try:
        assert sys.modules["pca"].PCA is PCA
        PCA.__module__ = "pca"                      # what a pickle of the reference's own class records
        try:
            torch.save(p, tmp_path / "pca.pt")
        finally:
            PCA.__module__ = "tokensgen_amd.pca"
        assert b"tokensgen_amd" not in (tmp_path / "pca.pt").read_bytes()
        q = torch.load(tmp_path / "pca.pt", weights_only=False)
        assert type(q) is PCA and torch.equal(q.components_, p.components_)
    finally:
        for k in [k for k in sys.modules if k == "longvgen" or k.startswith("longvgen.") or k == "pca"]:
            del sys.modules[k]


def test_scheduler_from_config_like_the_entry_script(tmp_path):
    """infer_cogvideo_mp_fifo.py:129,232 — from_config(existing.config, timestep_spacing="trailing"), also from a json file."""
    import json
    from tokensgen_amd.scheduler import CogVideoXDPMScheduler
    a = CogVideoXDPMScheduler(prediction_type="v_prediction", rescale_betas_zero_snr=True, snr_shift_scale=1.0)
    b = CogVideoXDPMScheduler.from_config(a.config, timestep_spacing="trailing")
    assert b.config.timestep_spacing == "trailing" and b.config.snr_shift_scale == 1.0 and torch.equal(a.alphas_cumprod, b.alphas_cumprod)
    b.set_timesteps(52)
    assert b.timesteps[0] == 999 and len(b.timesteps) == 52
    f = tmp_path / "scheduler_config.json"
    f.write_text(json.dumps(dict(_class_name="CogVideoXDPMScheduler", _diffusers_version="0.31.0", prediction_type="v_prediction",
                                 rescale_betas_zero_snr=True, snr_shift_scale=3.0, beta_schedule="scaled_linear")))
    c = CogVideoXDPMScheduler.from_config(str(f), timestep_spacing="trailing")
    assert c.config.snr_shift_scale == 3.0 and c.alphas_cumprod[-1] == 0.0


def test_resampler_checkpoint_roundtrip_and_set_pca(tmp_path):
    """Host side of the gen.yaml loading contract (infer_cogvideo_mp_fifo.py:113-118): Resampler.from_pretrained(dir, subfolder="resampler")
    reads what save_pretrained wrote; set_pca(path) unpickles a `pca.PCA` (resampler.py:201-207) and keeps its first 16 components; strict
    loading reports missing keys.  No kernel is launched (device "cpu" holds the tensors only)."""
    from oracle import resampler_ref as RR
    from tokensgen_amd import compat
    from tokensgen_amd.pca import PCA
    from tokensgen_amd.resampler import Resampler
    cfg = dict(dim=128, depth=2, dim_head=64, heads=2, num_height_queries=2, num_width_queries=3, num_temporal_queries=4, embedding_dim=128,
               output_dim=128, ff_mult=4, max_height_seq_len=4, max_width_seq_len=6, max_temporal_seq_len=5)
    sd = RR.make_state_dict(cfg, seed=1)
    r = Resampler(**cfg, device="cpu")
    r.load_state_dict(sd)
    assert sorted(r.expected_keys()) == sorted(sd)
    r.save_pretrained(str(tmp_path / "resampler"))
    r2 = Resampler.from_pretrained(str(tmp_path), subfolder="resampler", torch_dtype=torch.bfloat16, device="cpu").to("cpu")
    assert vars(r2.config) == vars(r.config)
    assert all(torch.equal(r2.state_dict()[k], v.to(torch.bfloat16)) for k, v in sd.items())
    with pytest.raises(RuntimeError, match="missing"):
        Resampler(**cfg, device="cpu").load_state_dict({k: v for k, v in sd.items() if k != "latents"})
    compat.ensure_pca_module()
    p = PCA(None).fit(torch.randn(300, 128, generator=torch.Generator().manual_seed(2)))
    torch.save(p, str(tmp_path / "pca.pt"))
    r2.set_pca(str(tmp_path / "pca.pt"))
    assert torch.equal(r2._pca_dev[0], p.components_[:16]) and torch.equal(r2._pca_dev[1], p.mean_.reshape(-1))
    r2.set_pca(None)
    assert r2.pca is None and r2._pca_dev is None
    with pytest.raises(ValueError, match="width"):
        Resampler(**dict(cfg, output_dim=256), device="cpu").set_pca(str(tmp_path / "pca.pt"))


def test_vae_param_shapes_match_the_diffusers_layout():
    from oracle import vae_ref as V
    from tokensgen_amd.vae import AutoencoderKLCogVideoX
    for cfg in (dict(block_out_channels=(128, 256, 256, 512), layers_per_block=3, latent_channels=16),
                dict(block_out_channels=(64, 128), layers_per_block=1, latent_channels=16)):
        vae = AutoencoderKLCogVideoX(block_out_channels=cfg["block_out_channels"], layers_per_block=cfg["layers_per_block"], device="cpu")
        assert vae.param_shapes() == {k: tuple(v.shape) for k, v in V.make_state_dict(cfg).items()}


def test_stratified_timestep_sampling_per_rank():
    """train_cogvideo_to2v.py:1797-1813 (`use_explicit_uniform_sampling`): rank r draws from its own stratum, rank 0 also covers the remainder."""
    import torch
    from tokensgen_amd.train import sample_timesteps
    g = torch.Generator().manual_seed(0)
    for world in (1, 3, 8):
        interval, shift = 1000 // world, 1000 % (1000 // world)
        seen = []
        for r in range(world):
            t = sample_timesteps(4096, 1000, r, world, explicit_uniform=True, generator=g)
            lo, hi = (0, interval + shift) if r == 0 else (r * interval + shift, (r + 1) * interval + shift)
            assert t.dtype == torch.int64 and int(t.min()) >= lo and int(t.max()) < hi
            seen.append((int(t.min()), int(t.max())))
        assert seen[0][0] == 0 and seen[-1][1] == 999            # 4096 draws per stratum of <= 1000 values: the ends are hit
    t = sample_timesteps(8192, 1000, 5, 8, explicit_uniform=False, generator=g)
    assert int(t.min()) == 0 and int(t.max()) == 999


CONV_PLAN_TABLE = """
    conv_in 8->128 8x240x360: in8 grid 1440 block 512 lds 56000 ksplit 1 reduce 0x0 case 0 splitk_floats 0
    conv_out 128->3 8x240x360: halo_narrow grid 1440 block 512 lds 126208 ksplit 1 reduce 0x0 case 0 splitk_floats 0
    conv_out 128->3 2x32x32: n16 grid 16 block 256 lds 65536 ksplit 1 reduce 0x0 case 0 splitk_floats 0
    128->128 8x240x360: halo2 grid 1440 block 512 lds 131072 ksplit 1 reduce 0x0 case 0 splitk_floats 0
    128->128 8x240x360 halo=0: w4_128 grid 1350 block 256 lds 163840 ksplit 1 reduce 0x0 case 0 splitk_floats 0
    256->256 8x120x180: w4_256 grid 675 block 256 lds 131072 ksplit 1 reduce 0x0 case 0 splitk_floats 0
    512->512 2x30x45: k128_splitk grid 440 block 256 lds 65536 ksplit 5 reduce 22x4 case 0 splitk_floats 6912000
    128->128 2x32x32: k128_splitk grid 96 block 256 lds 65536 ksplit 6 reduce 16x1 case 0 splitk_floats 1572864
    128->128 2x32x32 splitk=0: k128 grid 16 block 256 lds 65536 ksplit 1 reduce 0x0 case 0 splitk_floats 0
    128->128 1x240x544 (255 patches): k128 grid 1020 block 256 lds 65536 ksplit 1 reduce 0x0 case 0 splitk_floats 0
    128->128 1x256x512 (256 patches): halo2 grid 256 block 512 lds 131072 ksplit 1 reduce 0x0 case 0 splitk_floats 0
    conv_out 128->3 1x240x544 (255 patches): n16 grid 1020 block 256 lds 65536 ksplit 1 reduce 0x0 case 0 splitk_floats 0
    conv_out 128->3 1x256x512 (256 patches): halo_narrow grid 256 block 512 lds 126208 ksplit 1 reduce 0x0 case 0 splitk_floats 0
    128->128 256x1x1 (256 patches, 2 rows): k128_splitk grid 12 block 256 lds 65536 ksplit 6 reduce 2x1 case 0 splitk_floats 196608
    256->256 1x62x128 (31 tiles): k128_splitk grid 496 block 256 lds 65536 ksplit 4 reduce 62x2 case 4 splitk_floats 8126464
    256->256 1x64x128 (32 tiles): w4_256 grid 32 block 256 lds 131072 ksplit 1 reduce 0x0 case 0 splitk_floats 8388608
    128->2048 1x33x31 (M 1023): k128 grid 128 block 256 lds 65536 ksplit 1 reduce 0x0 case 0 splitk_floats 0
    128->2048 1x32x32 (M 1024): w4_256 grid 32 block 256 lds 131072 ksplit 1 reduce 0x0 case 0 splitk_floats 0
    128->128 1x23x89 (M 2047) w4=2: k128_splitk grid 96 block 256 lds 65536 ksplit 6 reduce 16x1 case 0 splitk_floats 1572096
    128->128 1x32x64 (M 2048) w4=2: w4_128 grid 4 block 256 lds 163840 ksplit 1 reduce 0x0 case 0 splitk_floats 1572864
    128->128 1x120x272 (255 tiles): k128_splitk grid 510 block 256 lds 65536 ksplit 2 reduce 255x1 case 2 splitk_floats 8355840
    128->128 1x128x256 (256 tiles): k128 grid 256 block 256 lds 65536 ksplit 1 reduce 0x0 case 0 splitk_floats 0
    128->128 2x32x32 halo=2: halo2 grid 4 block 512 lds 131072 ksplit 1 reduce 0x0 case 0 splitk_floats 1572864
    256->256 2x32x32 halo=2: halo2 grid 8 block 512 lds 131072 ksplit 1 reduce 0x0 case 0 splitk_floats 4194304
    conv_out 128->3 2x32x32 halo=2: halo_narrow grid 4 block 512 lds 126208 ksplit 1 reduce 0x0 case 0 splitk_floats 0
    256->256 1x32x32: k128_splitk grid 128 block 256 lds 65536 ksplit 8 reduce 8x2 case 8 splitk_floats 2097152
    256->256 1x32x32 w4=2: w4_256 grid 4 block 256 lds 131072 ksplit 1 reduce 0x0 case 0 splitk_floats 2097152
    refused: T = 0: error -2: tg_conv3d_cl: bad spatial shape
    refused: 8->64: error -2: tg_conv3d_cl: Cin = 8 is the 3x3x3, stride-1, 128-output-channel input convolution only
    refused: 8->128 100x2048x2048: error -2: tg_conv3d_cl: too many tiles
    refused: 8->128 2x1x1 with GroupNorm sums: error -2: tg_conv3d_cl: GroupNorm sums need at least as many 128-voxel rows (1) as 16 x 32 patches (2)
    refused: Cin 100: error -2: tg_conv3d_cl: need Cin%64==0 and cout_pad%128==0 (or cout_pad in {16, 32, ..., 112}) (Cin=100 cout=128 cout_pad=128)
    refused: kt 4: error -2: tg_conv3d_cl: unsupported kernel/stride/pad/up
    refused: 128->3 with GroupNorm sums: error -2: tg_conv3d_cl: fused GroupNorm sums need cout in {128, 256, 512, ...} (cout=3)
    refused: 128->7 (cout_pad 112) 4096x4096x4096: error -2: tg_conv3d_cl: too many tiles
    refused: 128->1024 4096x4096x4096: error -2: tg_conv3d_cl: too many tiles
    up2 256->256 8x120x180: up2_subpixel_shape_ok 1
    up2 256->512 1x33x31 (M 1023): up2_subpixel_shape_ok 0
    up2 256->512 1x32x32 (M 1024): up2_subpixel_shape_ok 1
    up2 256->256 1x28x64 (4 x 7 tiles): up2_subpixel_shape_ok 0
    up2 256->256 1x29x64 (4 x 8 tiles): up2_subpixel_shape_ok 1
"""


def test_conv_plan_table():
    """tokensgen_amd/csrc/conv_plan.h: which kernel, grid, block, LDS bytes and split-K form tg_conv3d_cl launches for a shape, and what
    tg_conv3d_splitk_floats / tg_conv3d_up2_subpixel_ok answer, as a pure host function printed by tests/conv_plan_table (tests/csrc/conv_plan_table.cpp:
    the cases; 256 CUs).  The expectations are worked out by hand from the dispatcher's conditions: the layers of the real workload, then a case on each side of
    every threshold — halo patches and 128 x 128 tiles against the CU count, 256-wide tiles against a eighth of it, M against 1024 and 2048, the knobs at 2
    below launch scale — and one refused shape per message (code -2 and text).  `reduce AxB case K` is the split-K reduce launch; splitk_floats is the
    128 x 128 kernel's workspace whether or not a halo or w4 kernel is taken first (callers cache it per shape)."""
    import subprocess
    exe = os.path.join(ROOT, "tests", "conv_plan_table")
    assert os.path.exists(exe), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    got, want = r.stdout.splitlines(), [ln.strip() for ln in CONV_PLAN_TABLE.strip().splitlines()]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w


def test_conv_kernel_query_follows_the_plan_and_the_knobs():
    """tg_conv3d_kernel / tg_conv3d_splitk_plan (lib.conv3d_kernel, lib.conv3d_splitk_plan): the live plan — conv_plan.h with the TG_CONV_* knobs as they are NOW and
    tg_device_cus(), which answers 256 without a device — agrees with lines of CONV_PLAN_TABLE above, and follows lib.debug_set and back."""
    from tokensgen_amd import lib as L
    q = lambda ci, co, cp, T, H, W, **kw: L.conv3d_kernel(T, H, W, ci, co, cp, 3, 3, 3, **kw)
    assert q(8, 128, 128, 8, 240, 360) == L.CONV_IN8 == 0
    assert q(128, 3, 16, 8, 240, 360) == L.CONV_HALO_NARROW == 1 and q(128, 3, 16, 2, 32, 32) == L.CONV_N16 == 2
    assert q(128, 128, 128, 8, 240, 360) == L.CONV_HALO2 == 3 and q(256, 256, 256, 8, 120, 180) == L.CONV_W4_256 == 4
    assert q(128, 128, 128, 1, 128, 256) == L.CONV_128 == 6 and q(512, 512, 512, 2, 30, 45) == L.CONV_128_SPLITK == 7
    plan = lambda ci, co, T, H, W: L.conv3d_splitk_plan(T, H, W, ci, co, co, 3, 3, 3)
    assert plan(512, 512, 2, 30, 45) == (5, 0) and plan(128, 128, 2, 32, 32) == (6, 0) and plan(256, 256, 1, 32, 32) == (8, 8) and plan(128, 128, 1, 120, 272) == (2, 2)
    assert L.conv3d_splitk_plan(1, 62, 128, 256, 256, 256, 1, 3, 3) == (4, 4) and plan(128, 128, 1, 128, 256) == (1, 0)
    # refused shapes: the plan's error code, whichever optional argument makes the shape illegal
    assert q(100, 128, 128, 2, 8, 8) == -2 and q(8, 64, 64, 2, 8, 8) == -2 and q(128, 3, 16, 2, 8, 8, gn_partial=True) == -2
    assert q(8, 128, 128, 2, 1, 1) == L.CONV_IN8 and q(8, 128, 128, 2, 1, 1, gn_partial=True) == -2 and q(8, 128, 128, 2, 8, 8, residual=True) == -2
    assert L.conv3d_kernel(2, 5, 6, 64, 128, 128, 1, 3, 3, up=2, out_dims=(4, 10, 12), t_map=True) == L.CONV_128
    # fused GroupNorm sums need whole groups per 128-channel tile: 384 channels (12 per group, 10.67 groups per tile) run, but not with the sums; 1024 (32 per group) do
    assert q(128, 384, 384, 2, 32, 32) == L.CONV_128_SPLITK and q(128, 384, 384, 2, 32, 32, gn_partial=True) == -2 and q(128, 640, 640, 2, 32, 32, gn_partial=True) == -2
    assert q(128, 1024, 1024, 2, 8, 8, gn_partial=True) == L.CONV_128 and q(128, 512, 512, 2, 8, 8, gn_partial=True) == L.CONV_128_SPLITK
    # the knobs, live: the shapes of the table's `halo=2`, `halo=0` and `w4=2` lines
    assert q(128, 128, 128, 2, 32, 32) == L.CONV_128_SPLITK and q(128, 3, 16, 2, 32, 32) == L.CONV_N16
    old = L.debug_set("TG_CONV_HALO", 2)
    try:
        assert old == 1 and q(128, 128, 128, 2, 32, 32) == L.CONV_HALO2 and q(256, 256, 256, 2, 32, 32) == L.CONV_HALO2 and q(128, 3, 16, 2, 32, 32) == L.CONV_HALO_NARROW
        assert plan(128, 128, 2, 32, 32) == (1, 0)
        L.debug_set("TG_CONV_HALO", 0)
        assert q(128, 128, 128, 8, 240, 360) == L.CONV_W4_128 == 5
    finally:
        L.debug_set("TG_CONV_HALO", old)
    assert q(128, 128, 128, 2, 32, 32) == L.CONV_128_SPLITK and q(128, 128, 128, 8, 240, 360) == L.CONV_HALO2
    assert q(256, 256, 256, 1, 32, 32) == L.CONV_128_SPLITK and q(128, 128, 128, 1, 32, 64) == L.CONV_128_SPLITK
    old = L.debug_set("TG_CONV_W4", 2)
    try:
        assert old == 1 and q(256, 256, 256, 1, 32, 32) == L.CONV_W4_256 and q(128, 128, 128, 1, 32, 64) == L.CONV_W4_128 and q(128, 128, 128, 1, 23, 89) == L.CONV_128_SPLITK
    finally:
        L.debug_set("TG_CONV_W4", old)
    assert q(256, 256, 256, 1, 32, 32) == L.CONV_128_SPLITK


GEMM_PLAN_TABLE = """
    plain 28326x3072->9216: k256w4 grid 256 block 256 lds 150784 group_m 4
    plain 28326x12288->3072: k256w4 grid 256 block 256 lds 150784 group_m 1
    plain 1024x8128->256: k256w4 grid 4 block 256 lds 150784 group_m 4
    plain 1024x8192->256: k256w4 grid 4 block 256 lds 150784 group_m 1
    plain 1023x256->256: k128 grid 16 block 256 lds 65536 group_m 0
    plain 1024x256->256: k256w4 grid 4 block 256 lds 150784 group_m 4
    plain 1024x256->384: k128 grid 24 block 256 lds 65536 group_m 0
    plain 1024x192->256: k256w8 grid 4 block 512 lds 131072 group_m 4
    plain 1024x256->256 w4=0: k256w8 grid 4 block 512 lds 131072 group_m 4
    plain 1024x256->256 lda 2^21-8: k256w4 grid 4 block 256 lds 150784 group_m 4
    plain 1024x256->256 lda 2^21: k256w8 grid 4 block 512 lds 131072 group_m 4
    plain 1024x256->256 ldw 2^21: k256w8 grid 4 block 512 lds 131072 group_m 4
    plain 2048x256->512 batch 2: k256w4 grid 32 block 256 lds 150784 group_m 4
    plain 65280x256->256 (255 tiles): k256w4 grid 255 block 256 lds 150784 group_m 4
    plain 65536x256->256 (256 tiles): k256w4 grid 256 block 256 lds 150784 group_m 4
    plain 65537x256->256 (257 tiles): k256w4 grid 256 block 256 lds 150784 group_m 4
    plain 1x512->18432: k128 grid 144 block 256 lds 65536 group_m 0
    plain 300x64->128 batch 3: k128 grid 9 block 256 lds 65536 group_m 0
    plain gate_res 1024x256->256: k256w4 grid 4 block 256 lds 150784 group_m 4
    plain gate_res 1000x256->256: k128 grid 16 block 256 lds 65536 group_m 0
    plain keep_gelu 1024x256->256: k256w4 grid 4 block 256 lds 150784 group_m 4
    plain gelu_grad 1024x256->256: k256w4 grid 4 block 256 lds 150784 group_m 4
    pair 1024+1280 x256->256: k256w4 grid 9 block 256 lds 150784 group_m 4
    pair 1024+1280 x64->256: k256w8 grid 9 block 512 lds 131072 group_m 4
    pair 1024+1280 x256->256 w4=0: k256w8 grid 9 block 512 lds 131072 group_m 4
    pair silu 1024+1280 x256->256: k256w4 grid 9 block 256 lds 150784 group_m 4
    qkv 1024x256->768 v_col0 512: k256w4 grid 12 block 256 lds 150784 group_m 4
    qkv 1024+1280 x256->768 v_col0 512: k256w4 grid 27 block 256 lds 150784 group_m 4
    lora 1024x256->256 R 64: k256w4 grid 4 block 256 lds 150784 group_m 4
    lora 1024x256->256 R 384: k256w4 grid 4 block 256 lds 150784 group_m 4
    lora 1024x8192->256 R 64: k256w4 grid 4 block 256 lds 150784 group_m 1
    refused: plain M = 0: error -2: tg_gemm_bf16: bad dims M=0 N=128 K=64 batch=1
    refused: plain N = 100: error -2: tg_gemm_bf16: need N%128==0 and K%64==0 (N=100 K=64)
    refused: plain K = 96: error -2: tg_gemm_bf16: need N%128==0 and K%64==0 (N=128 K=96)
    refused: plain epilogue 6: error -1: tg_gemm_bf16: unknown epilogue 6
    plain 2147483391x64->65536 (2^31 - 256 tiles): k256w8 grid 256 block 512 lds 131072 group_m 4
    refused: plain 2147483647x64->65536 (2^31 tiles): error -2: tg_gemm_bf16: too many tiles
    refused: plain keep_gelu M = 512: error -2: tg_gemm_bf16: the keep-GELU / GELU-grad epilogues exist in the 4-wave kernel only (M >= 1024, N%256 == 0, K >= 256)
    refused: plain keep_gelu K = 192: error -2: tg_gemm_bf16: the keep-GELU / GELU-grad epilogues exist in the 4-wave kernel only (M >= 1024, N%256 == 0, K >= 256)
    refused: plain keep_gelu N = 384: error -2: tg_gemm_bf16: the keep-GELU / GELU-grad epilogues exist in the 4-wave kernel only (M >= 1024, N%256 == 0, K >= 256)
    refused: plain keep_gelu w4=0: error -2: tg_gemm_bf16: the keep-GELU / GELU-grad epilogues exist in the 4-wave kernel only (M >= 1024, N%256 == 0, K >= 256)
    refused: plain gelu_grad M = 512: error -2: tg_gemm_bf16: the keep-GELU / GELU-grad epilogues exist in the 4-wave kernel only (M >= 1024, N%256 == 0, K >= 256)
    refused: plain gelu_grad K = 192: error -2: tg_gemm_bf16: the keep-GELU / GELU-grad epilogues exist in the 4-wave kernel only (M >= 1024, N%256 == 0, K >= 256)
    refused: plain gelu_grad N = 384: error -2: tg_gemm_bf16: the keep-GELU / GELU-grad epilogues exist in the 4-wave kernel only (M >= 1024, N%256 == 0, K >= 256)
    refused: plain gelu_grad w4=0: error -2: tg_gemm_bf16: the keep-GELU / GELU-grad epilogues exist in the 4-wave kernel only (M >= 1024, N%256 == 0, K >= 256)
    refused: pair M2 = 1023: error -2: tg_gemm_bf16_pair: both problems must be 256^2-kernel shapes (M >= 1024, N%256 == 0, K%64 == 0)
    refused: pair N = 384: error -2: tg_gemm_bf16_pair: both problems must be 256^2-kernel shapes (M >= 1024, N%256 == 0, K%64 == 0)
    refused: pair epilogue 3: error -1: tg_gemm_bf16_pair: bias / GELU / SiLU epilogues only
    refused: qkv K = 192: error -2: tg_gemm_bf16_qkv: needs the 4-wave kernel's shapes (M >= 1024, N%256 == 0, K%64 == 0, K >= 256)
    refused: qkv M = 1023: error -2: tg_gemm_bf16_qkv: needs the 4-wave kernel's shapes (M >= 1024, N%256 == 0, K%64 == 0, K >= 256)
    refused: qkv M2 = 512: error -2: tg_gemm_bf16_qkv: needs the 4-wave kernel's shapes (M >= 1024, N%256 == 0, K%64 == 0, K >= 256)
    refused: qkv v_col0 = 0: error -2: tg_gemm_bf16_qkv: v_col0 must be a multiple of 256 inside (0, N)
    refused: qkv v_col0 = N: error -2: tg_gemm_bf16_qkv: v_col0 must be a multiple of 256 inside (0, N)
    refused: qkv v_col0 = 384: error -2: tg_gemm_bf16_qkv: v_col0 must be a multiple of 256 inside (0, N)
    refused: qkv vt_ld = 1000: error -2: tg_gemm_bf16_qkv: vt_ld must be a multiple of 64 and >= M
    refused: qkv vt_ld = 960: error -2: tg_gemm_bf16_qkv: vt_ld must be a multiple of 64 and >= M
    refused: qkv lda = 2^21: error -2: tg_gemm_bf16_qkv: leading dimensions must be < 2^21 elements
    refused: qkv w4=0: error -1: tg_gemm_bf16_qkv: only the 4-wave GEMM kernel has the V^T epilogue (TG_GEMM_W4=0 is set)
    refused: lora M = 1023: error -2: tg_gemm_bf16_lora: needs the 4-wave kernel's shapes (M >= 1024, N%256 == 0, K%64 == 0, K >= 256): M=1023 N=256 K=256 batch=1
    refused: lora R = 32: error -2: tg_gemm_bf16_lora: the rank must be a multiple of 64 in 64..384 (R=32)
    refused: lora R = 96: error -2: tg_gemm_bf16_lora: the rank must be a multiple of 64 in 64..384 (R=96)
    refused: lora R = 448: error -2: tg_gemm_bf16_lora: the rank must be a multiple of 64 in 64..384 (R=448)
    refused: lora ldt = 56: error -2: tg_gemm_bf16_lora: leading dimensions must cover their rows and be < 2^21 elements
    refused: lora ldb = 2^21: error -2: tg_gemm_bf16_lora: leading dimensions must cover their rows and be < 2^21 elements
    refused: lora w4=0: error -2: tg_gemm_bf16_lora: only the 4-wave GEMM kernel has the low-rank tail (TG_GEMM_W4=0 is set)
"""


def test_gemm_plan_table():
    """tokensgen_amd/csrc/gemm_plan.h: which of the three GEMM kernels, grid, block, LDS bytes and group_m the four entry points of gemm.hip launch for a shape, and
    which shapes they refuse with which code and text, as a pure host function printed by tests/gemm_plan_table (tests/csrc/gemm_plan_table.cpp: the cases; 256 CUs;
    a case is named M x K -> N).  The workload's block projections, then a case on each side of every threshold: M against 1024, N a multiple of 128 only, K against
    256 and 8192, the knob, the leading dimensions against 2^21, the tiles against the CU count and against 2^31; then one refused shape per message on each side of its
    threshold.  TG_GEMM_W4 = 0 where only the 4-wave kernel will do is -1 from the qkv entry and -2 from the lora entry and the activation epilogues: the codes are ABI."""
    import subprocess
    exe = os.path.join(ROOT, "tests", "gemm_plan_table")
    assert os.path.exists(exe), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    got, want = r.stdout.splitlines(), [ln.strip() for ln in GEMM_PLAN_TABLE.strip().splitlines()]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w


def test_gemm_supported_predicates():
    """kernels.gemm_{act,lora,qkv,pair}_supported ask the library (tg_gemm_kernel: gemm_plan.h with the live TG_GEMM_W4 knob) instead of restating its rule.  The
    values below are what the hand-written conditions they replace answered, with the knob at 1 and at 0: the workload's shapes, M at 1023 / 1024, K at 192 / 256,
    N = 384, the rank at 32 / 64 / 384 / 448, a leading dimension at 2^21 - 8 / 2^21.  (act, lora: M, N, K[, R][, lda, ldw[, ldt, ldb]]; qkv: M, N, K, v_col0; pair:
    M1, M2, N, K.)"""
    from tokensgen_amd import kernels as K, lib as L
    P = 1 << 21
    T, F = True, False
    table = {       # helper: [(arguments, answer with TG_GEMM_W4 = 1, answer with TG_GEMM_W4 = 0)]
        K.gemm_act_supported: [
            ((28326, 12288, 3072), T, F), ((28326, 3072, 12288), T, F), ((17550, 12288, 3072), T, F), ((17776, 12288, 3072), T, F), ((1023, 256, 256), F, F),
            ((1024, 256, 256), T, F), ((1024, 256, 192), F, F), ((1024, 384, 256), F, F), ((300, 256, 256), F, F), ((1024, 256, 256, P - 8, P - 8), T, F),
            ((1024, 256, 256, P, 256), F, F), ((1024, 256, 256, 256, P), F, F), ((1024, 100, 256), F, F), ((1024, 256, 96), F, F)],
        K.gemm_lora_supported: [
            ((28326, 9216, 3072, 128), T, F), ((28326, 3072, 3072, 64), T, F), ((17550, 3072, 3072, 64), T, F), ((1024, 256, 256, 64), T, F),
            ((1023, 256, 256, 64), F, F), ((1024, 256, 192, 64), F, F), ((1024, 384, 256, 64), F, F), ((1024, 256, 256, 32), F, F), ((1024, 256, 256, 384), T, F),
            ((1024, 256, 256, 448), F, F), ((1024, 256, 256, 96), F, F), ((1024, 256, 256, 64, P - 8, P - 8, P - 8, P - 8), T, F),
            ((1024, 256, 256, 64, P, 256, 64, 64), F, F), ((1024, 256, 256, 64, 256, 256, P, 64), F, F), ((1024, 256, 256, 64, 256, 256, 64, P), F, F)],
        K.gemm_qkv_supported: [
            ((17776, 9216, 3072, 6144), T, F), ((28326, 9216, 3072, 6144), T, F), ((17550, 9216, 3072, 6144), T, F), ((1024, 768, 256, 512), T, F),
            ((1023, 768, 256, 512), F, F), ((1024, 768, 192, 512), F, F), ((1024, 384, 256, 256), F, F), ((1024, 768, 256, 384), F, F), ((1024, 768, 256, 256), T, F),
            ((300, 384, 128, 256), F, F)],
        K.gemm_pair_supported: [      # the pair entry takes either 256x256 kernel: the knob does not matter
            ((17776, 28326, 9216, 3072), T, T), ((17550, 17776, 9216, 3072), T, T), ((1024, 1280, 768, 256), T, T), ((1023, 1280, 768, 256), F, F),
            ((1024, 1280, 384, 256), F, F), ((1024, 1280, 768, 192), T, T), ((1024, 1024, 256, 64), T, T), ((300, 330, 384, 128), F, F)],
    }
    for knob in (1, 0):
        old = L.debug_set("TG_GEMM_W4", knob)
        try:
            for fn, cases in table.items():
                for case in cases:
                    assert fn(*case[0]) is case[2 - knob], (fn.__name__, case[0], knob)
        finally:
            L.debug_set("TG_GEMM_W4", old)


ATTENTION_PLAN_TABLE = """
    full 48x2 nq 17776 + rider 226: pp<1,1,0,0,0> grid 3328 block 512 lds 98304 both rows 0+17776 wgs 3360/3456 split 3232+128
    full 48x2 nq 17776 + rider 226: pp<1,1,0,0,1> grid 256 block 512 lds 98304 both rows 0+17776 wgs 3360/3456 split 3232+128
    full 48x2 nq 17776 + rider 226: combine(1) grid 512 block 256 lds 0 both rows 0+17776 wgs 3360/3456 split 3232+128
    full 48x2 nq 17776 + rider 226: pp<1,0,0,1,0> grid 256 block 512 lds 98304 both rows 0+17776 wgs 3360/3456 split 3232+128
    plain 48x2 nq 17776: pp<0,0,0,0,0> grid 3264 block 512 lds 98304 main rows 0+17408 wgs 3264/3264 split 3264+0
    plain 48x2 nq 17776: fwd<1> grid 288 block 256 lds 0 main rows 17408+368 wgs 0/0 split 0+0
    full 48x2 nq 9442: pp<1,1,0,0,0> grid 1728 block 512 lds 98304 main rows 0+9216 wgs 1728/1728 split 1728+0
    full 48x2 nq 9442: pp<1,0,0,1,0> grid 256 block 512 lds 98304 main rows 0+9216 wgs 1728/1728 split 1728+0
    full 48x2 nq 9442: fwd<1> grid 192 block 256 lds 0 main rows 9216+226 wgs 0/0 split 0+0
    plain lse 48x2 nq 17776: pp<0,0,1,0,0> grid 3264 block 512 lds 98304 main rows 0+17408 wgs 3264/3264 split 3264+0
    plain lse 48x2 nq 17776: fwd<1> grid 288 block 256 lds 0 main rows 17408+368 wgs 0/0 split 0+0
    full lse 48x2 nq 17776: pp<1,1,1,0,0> grid 3264 block 512 lds 98304 main rows 0+17408 wgs 3264/3264 split 3264+0
    full lse 48x2 nq 17776: pp<1,0,1,1,0> grid 256 block 512 lds 98304 main rows 0+17408 wgs 3264/3264 split 3264+0
    full lse 48x2 nq 17776: fwd<1> grid 288 block 256 lds 0 main rows 17408+368 wgs 0/0 split 0+0
    prescaled lse, no retry 48x2 nq 17776: pp<0,0,1,0,0> grid 3264 block 512 lds 98304 main rows 0+17408 wgs 3264/3264 split 3264+0
    prescaled lse, no retry 48x2 nq 17776: fwd<1> grid 288 block 256 lds 0 main rows 17408+368 wgs 0/0 split 0+0
    plain 48x2 nq 6806 2 segments: pp<0,0,0,0,0> grid 1248 block 512 lds 98304 main rows 0+6656 wgs 1248/1248 split 1248+0
    plain 48x2 nq 6806 2 segments: fwd<1> grid 192 block 256 lds 0 main rows 6656+150 wgs 0/0 split 0+0
    plain 2x2 nq 700: fwd<1> grid 24 block 256 lds 0 main rows 0+700 wgs 8/8 split 8+0
    plain 48x2 nq 2816: fwd<2> grid 1056 block 256 lds 0 main rows 0+2816 wgs 576/576 split 576+0
    plain 1x1 nq 523776 (1023 wgs): fwd<2> grid 2046 block 256 lds 0 main rows 0+523776 wgs 1023/1023 split 1023+0
    plain 1x1 nq 524288 (1024 wgs): pp<0,0,0,0,0> grid 1024 block 512 lds 98304 main rows 0+524288 wgs 1024/1024 split 1024+0
    plain 1x1 nq 523777 (1023 full + ragged): pp<0,0,0,0,0> grid 1024 block 512 lds 98304 main rows 0+523777 wgs 1024/1024 split 1024+0
    plain 2x2 nq 700 pp_min 1: pp<0,0,0,0,0> grid 8 block 512 lds 98304 main rows 0+700 wgs 8/8 split 8+0
    plain 1x1 nq 261888 (wg256 1023): fwd<1> grid 2046 block 256 lds 0 main rows 0+261888 wgs 512/512 split 512+0
    plain 1x1 nq 262144 (wg256 1024): fwd<2> grid 1024 block 256 lds 0 main rows 0+262144 wgs 512/512 split 512+0
    plain 48x2 nq 16996: pp<0,0,0,0,0> grid 3264 block 512 lds 98304 main rows 0+16996 wgs 3264/3264 split 3264+0
    plain 48x2 nq 17776 + rider 226: pp<0,0,0,0,0> grid 3456 block 512 lds 98304 both rows 0+17776 wgs 3360/3456 split 3456+0
    full 1x1 nq 524288 (R 0): pp<1,1,0,0,0> grid 1024 block 512 lds 98304 main rows 0+524288 wgs 1024/1024 split 1024+0
    full 1x1 nq 524288 (R 0): pp<1,0,0,1,0> grid 256 block 512 lds 98304 main rows 0+524288 wgs 1024/1024 split 1024+0
    full 1x1 nq 575488 (R 100): pp<1,1,0,0,0> grid 1024 block 512 lds 98304 main rows 0+575488 wgs 1124/1124 split 1024+100
    full 1x1 nq 575488 (R 100): pp<1,1,0,0,1> grid 208 block 512 lds 98304 main rows 0+575488 wgs 1124/1124 split 1024+100
    full 1x1 nq 575488 (R 100): combine(1) grid 400 block 256 lds 0 main rows 0+575488 wgs 1124/1124 split 1024+100
    full 1x1 nq 575488 (R 100): pp<1,0,0,1,0> grid 256 block 512 lds 98304 main rows 0+575488 wgs 1124/1124 split 1024+100
    full 1x1 nq 589824 (R 128): pp<1,1,0,0,0> grid 1024 block 512 lds 98304 main rows 0+589824 wgs 1152/1152 split 1024+128
    full 1x1 nq 589824 (R 128): pp<1,1,0,0,1> grid 256 block 512 lds 98304 main rows 0+589824 wgs 1152/1152 split 1024+128
    full 1x1 nq 589824 (R 128): combine(1) grid 512 block 256 lds 0 main rows 0+589824 wgs 1152/1152 split 1024+128
    full 1x1 nq 589824 (R 128): pp<1,0,0,1,0> grid 256 block 512 lds 98304 main rows 0+589824 wgs 1152/1152 split 1024+128
    full 1x1 nq 590336 (R 129): pp<1,1,0,0,0> grid 1153 block 512 lds 98304 main rows 0+590336 wgs 1153/1153 split 1153+0
    full 1x1 nq 590336 (R 129): pp<1,0,0,1,0> grid 256 block 512 lds 98304 main rows 0+590336 wgs 1153/1153 split 1153+0
    full 8x1 nq 8192 pp_min 1 (128 wgs): pp<1,1,0,0,0> grid 128 block 512 lds 98304 main rows 0+8192 wgs 128/128 split 128+0
    full 8x1 nq 8192 pp_min 1 (128 wgs): pp<1,0,0,1,0> grid 128 block 512 lds 98304 main rows 0+8192 wgs 128/128 split 128+0
    full 1x1 nq 131072 pp_min 1 (256 wgs): pp<1,1,0,0,0> grid 256 block 512 lds 98304 main rows 0+131072 wgs 256/256 split 256+0
    full 1x1 nq 131072 pp_min 1 (256 wgs): pp<1,0,0,1,0> grid 256 block 512 lds 98304 main rows 0+131072 wgs 256/256 split 256+0
    full 1x1 nq 131584 pp_min 1 (257 wgs): pp<1,1,0,0,0> grid 256 block 512 lds 98304 main rows 0+131584 wgs 257/257 split 256+1
    full 1x1 nq 131584 pp_min 1 (257 wgs): pp<1,1,0,0,1> grid 16 block 512 lds 98304 main rows 0+131584 wgs 257/257 split 256+1
    full 1x1 nq 131584 pp_min 1 (257 wgs): combine(1) grid 4 block 256 lds 0 main rows 0+131584 wgs 257/257 split 256+1
    full 1x1 nq 131584 pp_min 1 (257 wgs): pp<1,0,0,1,0> grid 256 block 512 lds 98304 main rows 0+131584 wgs 257/257 split 256+1
    full 1x1 nq 512 + rider 132608 pp_min 1 (R 4 > 1): pp<1,1,0,0,0> grid 260 block 512 lds 98304 both rows 0+512 wgs 1/260 split 260+0
    full 1x1 nq 512 + rider 132608 pp_min 1 (R 4 > 1): pp<1,0,0,1,0> grid 256 block 512 lds 98304 both rows 0+512 wgs 1/260 split 260+0
    full 1x1 nq 589824 nk 64: pp<1,1,0,0,0> grid 1152 block 512 lds 98304 main rows 0+589824 wgs 1152/1152 split 1152+0
    full 1x1 nq 589824 nk 64: pp<1,0,0,1,0> grid 256 block 512 lds 98304 main rows 0+589824 wgs 1152/1152 split 1152+0
    full 1x1 nq 589824 nk 65: pp<1,1,0,0,0> grid 1024 block 512 lds 98304 main rows 0+589824 wgs 1152/1152 split 1024+128
    full 1x1 nq 589824 nk 65: pp<1,1,0,0,1> grid 256 block 512 lds 98304 main rows 0+589824 wgs 1152/1152 split 1024+128
    full 1x1 nq 589824 nk 65: combine(1) grid 512 block 256 lds 0 main rows 0+589824 wgs 1152/1152 split 1024+128
    full 1x1 nq 589824 nk 65: pp<1,0,0,1,0> grid 256 block 512 lds 98304 main rows 0+589824 wgs 1152/1152 split 1024+128
    full 1x1 nq 589824 split floats 17039360: pp<1,1,0,0,0> grid 1024 block 512 lds 98304 main rows 0+589824 wgs 1152/1152 split 1024+128
    full 1x1 nq 589824 split floats 17039360: pp<1,1,0,0,1> grid 256 block 512 lds 98304 main rows 0+589824 wgs 1152/1152 split 1024+128
    full 1x1 nq 589824 split floats 17039360: combine(1) grid 512 block 256 lds 0 main rows 0+589824 wgs 1152/1152 split 1024+128
    full 1x1 nq 589824 split floats 17039360: pp<1,0,0,1,0> grid 256 block 512 lds 98304 main rows 0+589824 wgs 1152/1152 split 1024+128
    full 1x1 nq 589824 split floats 17039359: pp<1,1,0,0,0> grid 1152 block 512 lds 98304 main rows 0+589824 wgs 1152/1152 split 1152+0
    full 1x1 nq 589824 split floats 17039359: pp<1,0,0,1,0> grid 256 block 512 lds 98304 main rows 0+589824 wgs 1152/1152 split 1152+0
    full lse 1x1 nq 589824: pp<1,1,1,0,0> grid 1152 block 512 lds 98304 main rows 0+589824 wgs 1152/1152 split 1152+0
    full lse 1x1 nq 589824: pp<1,0,1,1,0> grid 256 block 512 lds 98304 main rows 0+589824 wgs 1152/1152 split 1152+0
    full 48x2 nq 17776 + rider 226 split 0: pp<1,1,0,0,0> grid 3456 block 512 lds 98304 both rows 0+17776 wgs 3360/3456 split 3456+0
    full 48x2 nq 17776 + rider 226 split 0: pp<1,0,0,1,0> grid 256 block 512 lds 98304 both rows 0+17776 wgs 3360/3456 split 3456+0
    full 48x2 nq 17776 + rider 226 fixedm 0: pp<1,0,0,0,0> grid 3328 block 512 lds 98304 both rows 0+17776 wgs 3360/3456 split 3232+128
    full 48x2 nq 17776 + rider 226 fixedm 0: pp<1,0,0,0,1> grid 256 block 512 lds 98304 both rows 0+17776 wgs 3360/3456 split 3232+128
    full 48x2 nq 17776 + rider 226 fixedm 0: combine(0) grid 512 block 256 lds 0 both rows 0+17776 wgs 3360/3456 split 3232+128
    full 48x2 nq 17776 + rider 226, a segment without bound: pp<1,0,0,0,0> grid 3328 block 512 lds 98304 both rows 0+17776 wgs 3360/3456 split 3232+128
    full 48x2 nq 17776 + rider 226, a segment without bound: pp<1,0,0,0,1> grid 256 block 512 lds 98304 both rows 0+17776 wgs 3360/3456 split 3232+128
    full 48x2 nq 17776 + rider 226, a segment without bound: combine(0) grid 512 block 256 lds 0 both rows 0+17776 wgs 3360/3456 split 3232+128
    full 48x2 nq 17776 + rider 226, no retry: pp<1,0,0,0,0> grid 3328 block 512 lds 98304 both rows 0+17776 wgs 3360/3456 split 3232+128
    full 48x2 nq 17776 + rider 226, no retry: pp<1,0,0,0,1> grid 256 block 512 lds 98304 both rows 0+17776 wgs 3360/3456 split 3232+128
    full 48x2 nq 17776 + rider 226, no retry: combine(0) grid 512 block 256 lds 0 both rows 0+17776 wgs 3360/3456 split 3232+128
    full 48x2 nq 17776 + rider 226, not prescaled: pp<0,0,0,0,0> grid 3328 block 512 lds 98304 both rows 0+17776 wgs 3360/3456 split 3232+128
    full 48x2 nq 17776 + rider 226, not prescaled: pp<0,0,0,0,1> grid 256 block 512 lds 98304 both rows 0+17776 wgs 3360/3456 split 3232+128
    full 48x2 nq 17776 + rider 226, not prescaled: combine(0) grid 512 block 256 lds 0 both rows 0+17776 wgs 3360/3456 split 3232+128
    full 48x4 nq 3172: pp<1,1,0,0,0> grid 1024 block 512 lds 98304 main rows 0+3072 wgs 1152/1152 split 1024+128
    full 48x4 nq 3172: pp<1,1,0,0,1> grid 256 block 512 lds 98304 main rows 0+3072 wgs 1152/1152 split 1024+128
    full 48x4 nq 3172: combine(1) grid 512 block 256 lds 0 main rows 0+3072 wgs 1152/1152 split 1024+128
    full 48x4 nq 3172: pp<1,0,0,1,0> grid 256 block 512 lds 98304 main rows 0+3072 wgs 1152/1152 split 1024+128
    full 48x4 nq 3172: fwd<1> grid 192 block 256 lds 0 main rows 3072+100 wgs 0/0 split 0+0
    plain 2x2 nq 700 + rider 226: fwd<1> grid 24 block 256 lds 0 main rows 0+700 wgs 8/8 split 8+0
    plain 2x2 nq 700 + rider 226: fwd<1> grid 8 block 256 lds 0 rider rows 0+226 wgs 4/4 split 4+0
    full 48x2 nq 2816 + rider 17776: fwd<2> grid 1056 block 256 lds 0 main rows 0+2816 wgs 576/576 split 576+0
    full 48x2 nq 2816 + rider 17776: pp<1,0,0,0,0> grid 3264 block 512 lds 98304 rider rows 0+17408 wgs 3264/3264 split 3264+0
    full 48x2 nq 2816 + rider 17776: fwd<1> grid 288 block 256 lds 0 rider rows 17408+368 wgs 0/0 split 0+0
    fwd nq 0: error -2: tg_attention_fwd: bad shape nq=0 nk1=64
    fwd nq 1: ok
    fwd nk1 0: error -2: tg_attention_fwd: bad shape nq=64 nk1=0
    fwd heads 0: error -2: tg_attention_fwd: bad shape nq=64 nk1=64
    fwd batch 0: error -2: tg_attention_fwd: bad shape nq=64 nk1=64
    multi 1x1 nq 1 nk 1: ok
    multi heads 0: error -2: tg_attention_fwd_multi: bad shape
    multi batch 0: error -2: tg_attention_fwd_multi: bad shape
    multi nq 0: error -1: tg_attention_fwd_multi: problem 0
    multi nseg 0: error -1: tg_attention_fwd_multi: problem 0
    multi nseg 2: ok
    multi nseg 3: error -1: tg_attention_fwd_multi: problem 0
    multi segment 1 nk 0: error -2: tg_attention: problem 0 segment 1: nk=0
    multi segment 2 nk 0: error -2: tg_attention: problem 0 segment 2: nk=0
    multi segment 1 nk 64 vt_ld 64: ok
    multi segment 1 nk 65 vt_ld 64: error -2: tg_attention: problem 0 segment 1: vt_ld must cover nk rounded up to 64
    multi segment 1 nk 65 vt_ld 128: ok
    multi segment 2 nk 65 vt_ld 64: error -2: tg_attention: problem 0 segment 2: vt_ld must cover nk rounded up to 64
    multi per-item scales batch 16: ok
    multi per-item scales batch 17: error -2: tg_attention_fwd_multi: per-item segment-2 scales for at most 16 batch items (got 17)
    multi one scale batch 17: ok
    multi rider nq 1: ok
    multi rider nq 0: error -1: tg_attention_fwd_multi: problem 1 must have one key segment
    multi rider nseg 2: error -1: tg_attention_fwd_multi: problem 1 must have one key segment
    multi rider nk 0: error -2: tg_attention: problem 1: nk=0
    multi rider nk 65 vt_ld 64: error -2: tg_attention: problem 1: vt_ld must cover nk rounded up to 64
    multi 48x2 nq 17776 + rider 226 retry 3457: ok
    multi 48x2 nq 17776 + rider 226 retry 3456: error -2: tg_attention_fwd_multi: retry workspace of 3456 ints, need 3457 (tg_attention_retry_ints)
    lse nq 1: ok
    lse nq 0: error -2: tg_attention_fwd_lse: bad shape nq=0 nk=64
    lse nk 0: error -2: tg_attention_fwd_lse: bad shape nq=64 nk=0
    lse nk 65 vt_ld 64: error -2: tg_attention: segment: vt_ld must cover nk rounded up to 64
    lse_ex heads 0: error -2: tg_attention_fwd_lse_ex: bad shape nq=64 nk=64
    lse_ex batch 0: error -2: tg_attention_fwd_lse_ex: bad shape nq=64 nk=64
    lse_ex 48x2 nq 17776 retry 3361: ok
    lse_ex 48x2 nq 17776 retry 3360: error -2: tg_attention_fwd_lse_ex: retry workspace of 3360 ints, need 3361 (tg_attention_retry_ints)
    layout nq 17776 nk 17776 heads 48 batch 2: seed 0 lse 6825984 d 8532480 cnt 10238984 ncnt 1708032 xmask 11947016 dq_part 11947112 total 11947120
    layout nq 480 nk 18256 heads 48 batch 2: seed 0 lse 184320 d 230400 cnt 276488 ncnt 46080 xmask 322568 dq_part 322664 total 23915636
    layout nq 1 nk 1 heads 1 batch 1: seed 0 lse 4 d 5 cnt 16 ncnt 32 xmask 48 dq_part 52 total 571
    layout nq 33 nk 7 heads 3 batch 1: seed 0 lse 396 d 495 cnt 604 ncnt 192 xmask 796 dq_part 800 total 51497
    layout nq 65536 nk 64 heads 1 batch 1: seed 0 lse 262144 d 327680 cnt 393224 ncnt 65536 xmask 458760 dq_part 458764 total 34013205
    layout nq 65537 nk 64 heads 1 batch 1: seed 0 lse 262148 d 327685 cnt 393232 ncnt 65568 xmask 458800 dq_part 458804 total 458807
    48x2 17776x17776 flag: problem 0: one kernel stats 70x96 wgs_k 6720 kparts 1 dq 0 join 0
    48x2 17776x17776 flag: fused grid 6720 block 512 lds 116736 main 0 rider -1 main_wgs 6720
    48x2 17776x17776: problem 0: two launches stats 70x96 wgs_k 6720 kparts 1 dq 6720 join 0
    48x2 17776x17776 flag dq unaligned: problem 0: two launches stats 70x96 wgs_k 6720 kparts 1 dq 6720 join 0
    47x2 17776x17776 flag: problem 0: two launches stats 70x94 wgs_k 6580 kparts 1 dq 6580 join 0
    48x2 8928x17776 flag (279 tiles): problem 0: two launches stats 35x96 wgs_k 6720 kparts 1 dq 3360 join 0
    48x2 8929x17776 flag (280 tiles): problem 0: one kernel stats 35x96 wgs_k 6720 kparts 1 dq 0 join 0
    48x2 8929x17776 flag (280 tiles): fused grid 6720 block 512 lds 116736 main 0 rider -1 main_wgs 6720
    48x2 480x18256 flag: problem 0: two launches stats 2x96 wgs_k 6912 kparts 8 dq 1536 join 2880
    48x2 480x18256 dq unaligned: problem 0: two launches stats 2x96 wgs_k 6912 kparts 1 dq 192 join 0
    32x8 256x4096 (256 blocks): problem 0: two launches stats 1x256 wgs_k 4096 kparts 6 dq 1536 join 4096
    257x1 256x4096 (257 blocks): problem 0: two launches stats 1x257 wgs_k 4112 kparts 1 dq 257 join 0
    48x2 480x1536 (48 key tiles): problem 0: two launches stats 2x96 wgs_k 576 kparts 3 dq 576 join 2880
    48x2 480x992 (31 key tiles): problem 0: two launches stats 2x96 wgs_k 384 kparts 1 dq 192 join 0
    48x2 main + vip-key flag: problem 0: one kernel stats 70x96 wgs_k 6720 kparts 1 dq 0 join 0
    48x2 main + vip-key flag: problem 1: one kernel stats 70x96 wgs_k 192 kparts 1 dq 0 join 0
    48x2 main + vip-key flag: fused grid 6912 block 512 lds 116736 main 0 rider 1 main_wgs 6720
    48x2 main + vip-query flag: problem 0: one kernel stats 70x96 wgs_k 6720 kparts 1 dq 0 join 0
    48x2 main + vip-query flag: problem 1: two launches stats 2x96 wgs_k 6912 kparts 8 dq 1536 join 2880
    48x2 main + vip-query flag: fused grid 6720 block 512 lds 116736 main 0 rider -1 main_wgs 6720
    48x2 vip-query + main flag: problem 0: two launches stats 2x96 wgs_k 6912 kparts 8 dq 1536 join 2880
    48x2 vip-query + main flag: problem 1: one kernel stats 70x96 wgs_k 6720 kparts 1 dq 0 join 0
    48x2 vip-query + main flag: fused grid 6720 block 512 lds 116736 main 1 rider -1 main_wgs 6720
    48x2 main + vip-key: problem 0: two launches stats 70x96 wgs_k 6720 kparts 1 dq 6720 join 0
    48x2 main + vip-key: problem 1: two launches stats 70x96 wgs_k 192 kparts 1 dq 6720 join 0
"""


def test_attention_plan_table():
    """tokensgen_amd/csrc/attention_plan.h: the launches of the forward entry points (kernel, grid, block, LDS bytes, the rows covered, the derived AttnParams fields:
    `wgs main_wgs/total_wgs`, `split split_first+nsplit`), the shapes they refuse (code and text), every offset of the backward's workspace, and the backward's form and
    grids, as pure host functions printed by tests/attention_plan_table (tests/csrc/attention_plan_table.cpp: the cases; 256 CUs).  The expectations are worked out by
    hand from the conditions of the launchers this header replaced: the workload's shapes, then a case on each side of every threshold — 1024 workgroups of 512 and of
    256 rows, the ragged tail with and without a saved round and with a rider, the split remainder at 0 / 128 / 129 and a launch within one round, one / two key tiles,
    the split workspace one float short, every condition of the constant shift — and for the backward the one-kernel conditions, the dQ split and its clamps, and two
    problems.  pp<PRESCALED,FIXEDM,LSE,RETRY,SPLIT>; the running-max log-sum-exp kernel is pp<0,0,1,0,0> for prescaled K too (scale_log2 is 1 there)."""
    import subprocess
    exe = os.path.join(ROOT, "tests", "attention_plan_table")
    assert os.path.exists(exe), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    got, want = r.stdout.splitlines(), [ln.strip() for ln in ATTENTION_PLAN_TABLE.strip().splitlines()]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w


def test_attention_size_functions_keep_their_formulas():
    """tg_attention_retry_ints, tg_attention_split_floats and tg_attention_bwd_ws_floats answer from attention_plan.h; callers allocate by them.  Held here to the
    formulas the three functions had before, written out (256 CUs: what the library assumes without a GPU, and the MI355X's count), around the thresholds: query rows at
    multiples of 512, 256 and 32 and one to each side, launches of at most one round, remainders at 0 / 128 / 129, the dQ partials at 256 / 257 query blocks."""
    from tokensgen_amd import lib as L
    lib = L.load()
    n_cu = 256
    half = 512 * (64 + 2 + 64)

    def wgs(nq0, nq1, heads, batch):
        return ((nq0 + 511) // 512 + ((nq1 + 511) // 512 if nq1 > 0 else 0)) * heads * batch

    def retry_ints(nq0, nq1, heads, batch):
        return 1 + wgs(nq0, nq1, heads, batch)

    def split_floats(nq0, nq1, heads, batch):
        g = wgs(nq0, nq1, heads, batch)
        R = g % n_cu
        return 2 * R * half if (g > n_cu and R > 0 and 2 * R <= n_cu) else 0

    def bwd_ws_floats(nq, nk, heads, batch):
        split = (nq + 255) // 256 * heads * batch <= 256
        return (6 * batch * heads * nq + 8 + batch * heads * ((nq + 31) // 32) * 32 + 8 + batch * heads + (8 * batch * nq * heads * 64 + 4 if split else 0))

    fwd = [(17776, 226, 48, 2), (17776, 0, 48, 2), (17550, 226, 48, 2), (9442, 0, 48, 2), (6806, 0, 48, 2), (700, 0, 2, 2), (700, 226, 2, 2), (2816, 0, 48, 2),
           (1, 0, 1, 1), (1, 1, 1, 1), (512, 0, 1, 1), (513, 0, 1, 1), (511, 512, 3, 5), (512, -3, 7, 1),
           (131072, 0, 1, 1), (131073, 0, 1, 1), (130560, 512, 1, 1), (131072, 512, 1, 1),                   # 256 / 257 workgroups: within one round or not
           (524288, 0, 1, 1), (575488, 0, 1, 1), (589312, 0, 1, 1), (589824, 0, 1, 1), (590336, 0, 1, 1),     # R = 0, 100, 127, 128, 129
           (512 * 12, 0, 48, 4), (3172, 0, 48, 4), (512 * 128, 0, 8, 1), (512 * 144, 0, 8, 1), (512 * 145, 0, 8, 1), (512 * 144, 8 * 512, 8, 1),
           (17776, 17776, 48, 2), (512, 132608, 1, 1), (4096, 4096, 24, 1)]
    for case in fwd:
        assert lib.tg_attention_retry_ints(*case) == retry_ints(*case), case
        assert lib.tg_attention_split_floats(*case) == split_floats(*case), case
    assert lib.tg_attention_split_floats(17776, 226, 48, 2) == 2 * 128 * half and lib.tg_attention_split_floats(589824, 0, 1, 1) == 2 * 128 * half
    assert lib.tg_attention_split_floats(590336, 0, 1, 1) == 0 and lib.tg_attention_split_floats(131072, 0, 1, 1) == 0
    bwd = [(17776, 17776, 48, 2), (480, 18256, 48, 2), (17776, 480, 48, 2), (17550, 17550, 48, 2), (1, 1, 1, 1), (2, 1, 1, 1), (3, 5, 1, 1), (31, 7, 3, 1), (32, 7, 3, 1),
           (33, 7, 3, 1), (255, 64, 2, 3), (256, 64, 2, 3), (257, 64, 2, 3), (65536, 64, 1, 1), (65537, 64, 1, 1), (256, 4096, 32, 8), (256, 4096, 257, 1),
           (257, 4096, 32, 4), (257, 4096, 32, 5), (512, 100, 128, 1), (513, 100, 128, 1), (300, 330, 6, 2), (700, 700, 2, 2), (8928, 17776, 48, 2), (8929, 17776, 48, 2)]
    for case in bwd:
        assert lib.tg_attention_bwd_ws_floats(*case) == bwd_ws_floats(*case), case
    assert lib.tg_attention_bwd_ws_floats(17776, 17776, 48, 2) == 11947120 and lib.tg_attention_bwd_ws_floats(480, 18256, 48, 2) == 23915636
