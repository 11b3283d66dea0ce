"""CogVideoXDDIMScheduler host side against runs of the reference class stored in tests/golden/scheduler_ddim.pt: tables, timestep
lists, the fp64 coefficient row, and the torch restatement (tests/ddim_ref.py) that the GPU tests use as their reference."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from ddim_ref import ddim_ref
from tokensgen_amd.scheduler import CogVideoXDDIMScheduler, CogVideoXDPMScheduler, ddim_coef_row

KW = dict(prediction_type="v_prediction", rescale_betas_zero_snr=True, snr_shift_scale=1.0, timestep_spacing="trailing")


@pytest.fixture(scope="module")
def gold(golden_dir):
    return torch.load(os.path.join(golden_dir, "scheduler_ddim.pt"), weights_only=False)


def test_tables_and_timesteps_equal_the_reference(gold):
    for one in (True, False):
        s, g = CogVideoXDDIMScheduler(set_alpha_to_one=one, **KW), gold["tables"][one]
        assert torch.equal(s.alphas_cumprod, g["alphas_cumprod"]) and torch.equal(s.betas, g["betas"])
        assert torch.equal(s.final_alpha_cumprod.double(), g["final_alpha_cumprod"].double())
        assert s.order == 1 and s.init_noise_sigma == 1.0 and len(s) == 1000 and s.config.set_alpha_to_one is one
    assert float(CogVideoXDDIMScheduler(**KW).final_alpha_cumprod) == 1.0
    for tag, n, kw in (("trailing50", 50, {}), ("trailing52", 52, {}), ("leading50_offset0", 50, dict(timestep_spacing="leading")),
                       ("leading50_offset1", 50, dict(timestep_spacing="leading", steps_offset=1)), ("linspace7", 7, dict(timestep_spacing="linspace"))):
        s = CogVideoXDDIMScheduler(**dict(KW, **kw))
        s.set_timesteps(n)
        assert torch.equal(s.timesteps, gold["timesteps"][tag]) and s.timesteps.dtype == torch.int64, tag
    assert gold["timesteps"]["trailing50"].tolist() == list(range(999, 0, -20))


@pytest.mark.parametrize("kw", [KW, dict(), dict(snr_shift_scale=3.0, rescale_betas_zero_snr=True, prediction_type="epsilon"),
                                dict(num_train_timesteps=500, beta_start=0.001, beta_end=0.02)])
def test_alphas_cumprod_is_the_dpm_table(kw):
    a, b = CogVideoXDDIMScheduler(**kw), CogVideoXDPMScheduler(**kw)
    assert torch.equal(a.alphas_cumprod, b.alphas_cumprod) and torch.equal(a.betas, b.betas) and vars(a.config) == vars(b.config)


def test_coef_row_reproduces_the_fp64_steps(gold):
    """x0 = sa x - sb v | (x - sb eps) / sa | v, prev = m1 x - m2 x0 in fp64 against the reference's all-fp64 `step`; the tolerances of
    tests/test_host_cpu.py for the DPM rows."""
    n = 0
    for c in gold["steps"]:
        if c["dtypes"] != "f64":
            continue
        tab = gold["tables"][c["set_alpha_to_one"]]
        row = ddim_coef_row(tab["alphas_cumprod"].numpy(), c["t"], c["prev_t"], float(tab["final_alpha_cumprod"]))
        sa, sb, m1, m2 = row[:4]
        assert row[4:] == [0.0, 0.0, 0.0, 0.0]
        i = gold["inputs"][c["row"]]
        x, v = i["sample"].double().numpy(), i["model_output"].double().numpy()
        x0 = {"v_prediction": lambda: sa * x - sb * v, "epsilon": lambda: (x - sb * v) / sa, "sample": lambda: v}[c["prediction_type"]]()
        assert np.allclose(x0, c["x0"].numpy(), rtol=1e-12, atol=1e-14), (c["t"], c["prediction_type"])
        assert np.allclose(m1 * x - m2 * x0, c["prev_sample"].numpy(), rtol=1e-12, atol=1e-14), (c["t"], c["prediction_type"])
        n += 1
    assert n == 14


def test_coef_row_edges(gold):
    ac = gold["tables"][True]["alphas_cumprod"].numpy()
    first = ddim_coef_row(ac, 999, 979, 1.0)
    assert first[0] == 0.0 and first[1] == 1.0 and first[2] == float(np.sqrt(1 - ac[979]))
    last = ddim_coef_row(ac, 19, -1, 1.0)
    assert last[2] == 0.0 and last[3] == -1.0
    other = ddim_coef_row(ac, 19, -1, float(ac[0]))                      # set_alpha_to_one=False: a small step is left
    assert other[2] > 0.0 and other[3] != -1.0
    bad = ac.copy()
    bad[5] = 1.0                                                         # 1 - a_t = 0: A = inf
    with pytest.raises(ValueError, match="non-finite"):
        ddim_coef_row(bad, 5, 3, 1.0)
    s = CogVideoXDDIMScheduler(**KW)
    t = s.coef_table([999, 19], [979, -1], "cpu")
    assert t.shape == (2, 8) and t.dtype == torch.float32 and t[:, 4:].abs().max() == 0 and t[1, 3] == -1.0
    assert torch.equal(s._get_variance(499, 479), ((1 - s.alphas_cumprod[479]) / (1 - s.alphas_cumprod[499])) * (1 - s.alphas_cumprod[499] / s.alphas_cumprod[479]))


def test_restatement_is_bitwise_the_reference_step(gold):
    """tests/ddim_ref.py with torch's own promotion against every recorded fp32-model-output and all-bf16 step: not one bit apart."""
    n = 0
    for c in gold["steps"]:
        i = gold["inputs"][c["row"]]
        tab = gold["tables"][c["set_alpha_to_one"]]
        tables = (tab["alphas_cumprod"], tab["final_alpha_cumprod"])
        if c["dtypes"] == "f32_bf16":
            mo, x, want = i["model_output"].bfloat16().float(), i["sample"].bfloat16(), torch.float32
        elif c["dtypes"] == "bf16":
            mo, x, want = i["model_output"].bfloat16(), i["sample"].bfloat16(), torch.bfloat16
        else:
            mo, x, want = i["model_output"].double(), i["sample"].double(), torch.float64
        prev, x0 = ddim_ref(mo, c["t"], c["prev_t"], x, tables, c["prediction_type"])
        assert prev.dtype == c["prev_sample"].dtype == want and x0.dtype == c["x0"].dtype == want
        assert torch.equal(prev, c["prev_sample"]) and torch.equal(x0, c["x0"]), (c["t"], c["prediction_type"], c["dtypes"])
        n += 1
    assert n == 42


def test_add_noise_and_get_velocity(gold):
    s = CogVideoXDDIMScheduler(**KW)
    for c in gold["train"]:
        noisy, vel = s.add_noise(c["sample"], c["noise"], c["timesteps"]), s.get_velocity(c["sample"], c["noise"], c["timesteps"])
        assert noisy.dtype == c["noisy"].dtype and torch.equal(noisy, c["noisy"]) and torch.equal(vel, c["velocity"]), c["dtype"]


def test_errors():
    s = CogVideoXDDIMScheduler(**KW)
    with pytest.raises(ValueError, match="cannot be larger"):
        s.set_timesteps(1001)
    x = torch.zeros(1, 1, 16, 4, 6, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="set_timesteps"):
        CogVideoXDDIMScheduler(**KW).step(x, 999, 979, x)
    with pytest.raises(ValueError, match="prediction_type"):
        CogVideoXDDIMScheduler(**dict(KW, prediction_type="flow"))
    with pytest.raises(NotImplementedError):
        CogVideoXDDIMScheduler(beta_schedule="linear")
    s.set_timesteps(50)
    with pytest.raises(ValueError, match="bf16"):                         # an fp32 model output that is not the .float() of a bf16 tensor
        s.step(torch.full((1, 1, 16, 4, 6), 1.0 + 2.0 ** -20), 999, 979, x)


def test_from_config_and_alias(tmp_path):
    dpm = CogVideoXDPMScheduler(**dict(KW, timestep_spacing="leading"))
    s = CogVideoXDDIMScheduler.from_config(dpm.config, timestep_spacing="trailing")
    assert isinstance(s, CogVideoXDDIMScheduler) and s.config.timestep_spacing == "trailing" and s.config.prediction_type == "v_prediction"
    assert s.config.rescale_betas_zero_snr is True and torch.equal(s.alphas_cumprod, dpm.alphas_cumprod)
    p = tmp_path / "scheduler_config.json"
    p.write_text(json.dumps(dict(_class_name="CogVideoXDPMScheduler", _diffusers_version="0.30.0", set_alpha_to_one=False, **KW)))
    s = CogVideoXDDIMScheduler.from_config(str(p))
    assert isinstance(s, CogVideoXDDIMScheduler) and s.config.set_alpha_to_one is False and s.final_alpha_cumprod == s.alphas_cumprod[0]
    # the DPM class built from a file that names the DDIM class (what CogVideoX-5b ships) is unchanged
    assert isinstance(CogVideoXDPMScheduler.from_config(dict(_class_name="CogVideoXDDIMScheduler", **KW)), CogVideoXDPMScheduler)
    from tokensgen_amd import compat
    saved = {k: v for k, v in sys.modules.items() if k == "longvgen" or k.startswith("longvgen.") or k == "pca"}
    try:
        compat.install_longvgen_alias(force=True)
        from longvgen.schedulers import CogVideoXDDIMScheduler as aliased
        assert aliased is CogVideoXDDIMScheduler
    finally:
        for k in [k for k in sys.modules if k == "longvgen" or k.startswith("longvgen.")]:
            del sys.modules[k]
        sys.modules.update(saved)
