"""Torch restatement of the deterministic DDIM step, written from its formulas (DDIM paper eq. 12 with sigma = 0, in the form the
scheduler uses): with a = alphas_cumprod[t], a_prev = alphas_cumprod[prev_t] (or final_alpha_cumprod when prev_t < 0)

    x0   = sqrt(a) x - sqrt(1 - a) v         v-prediction
         = (x - sqrt(1 - a) eps) / sqrt(a)   epsilon
         = model_output                      sample
    A    = sqrt((1 - a_prev) / (1 - a)),   B = sqrt(a_prev) - sqrt(a) A
    prev = A x + B x0

The coefficients stay 0-dim fp64 tensors and every product is a plain torch op, so torch's own type promotion does the rounding: a 0-dim
tensor does not promote a dimensioned one, hence bf16(coef) * bf16 tensor -> bf16, fp64 coef * fp32 tensor -> fp32, bf16 + fp32 -> fp32.
"""
import torch


def ddim_ref(model_output, t, prev_t, sample, tables, prediction_type):
    """tables = (alphas_cumprod [T] fp64, final_alpha_cumprod 0-dim).  Returns (prev_sample, x0) on model_output's device."""
    ac, final = tables
    a = ac[int(t)]
    a_prev = ac[int(prev_t)] if int(prev_t) >= 0 else final
    if prediction_type == "v_prediction":
        x0 = a ** 0.5 * sample - (1 - a) ** 0.5 * model_output
    elif prediction_type == "epsilon":
        x0 = (sample - (1 - a) ** 0.5 * model_output) / a ** 0.5
    elif prediction_type == "sample":
        x0 = model_output
    else:
        raise ValueError(prediction_type)
    A = ((1 - a_prev) / (1 - a)) ** 0.5
    B = a_prev ** 0.5 - a ** 0.5 * A
    return A * sample + B * x0, x0


def terms_magnitude(model_output, t, prev_t, sample, tables, prediction_type):
    """Sum of the absolute values of the terms of x0 and of prev (fp64), the `mag` of the per-element error bounds: (mag_x0, mag_prev)."""
    ac, final = tables
    a = float(ac[int(t)])
    a_prev = float(ac[int(prev_t)]) if int(prev_t) >= 0 else float(final)
    x, v = sample.double().abs(), model_output.double().abs()
    if prediction_type == "v_prediction":
        m0 = a ** 0.5 * x + (1 - a) ** 0.5 * v
    elif prediction_type == "epsilon":
        m0 = (x + (1 - a) ** 0.5 * v) / a ** 0.5
    else:
        m0 = v
    A = ((1 - a_prev) / (1 - a)) ** 0.5
    B = a_prev ** 0.5 - a ** 0.5 * A
    return m0, abs(A) * x + abs(B) * m0
