"""Keras' Adam(amsgrad=True) (TF 2.1: ApplyAdamWithAmsgrad, and Adam._resource_apply_sparse with amsgrad) restated in float64 on float32
hyper-parameters, as keras_adam64 of tests/test_optim_gpu.py restates ApplyAdam, and the one relation of the rule that is exact in
fp32: vhat' = where(vhat < v', v', vhat).  Restated, not run: parity with TensorFlow is unpinned, like the rest of oracle/.

    t = iterations + 1;  alpha = lr sqrt(1 - b2^t) / (1 - b1^t)
    m += (g - m)(1 - b1);  v += (g g - v)(1 - b2);  vhat = (vhat < v) ? v : vhat;  p -= (m alpha) / (sqrt(vhat) + eps)

The numeric tests take beta_2 = 0.5 and per-step gradient scales SCALES: with Keras' 0.999 an implementation that ignores vhat is only
4e-4 ... 1e-3 (norm-relative, five steps) away from the rule, too close to the bars to prove anything; with these inputs vhat > v on
most elements after steps 2, 3 and 5 and such an implementation is 0.19 ... 0.83 away."""
import numpy as np

SLOT_NAMES = ("m", "v", "vhat")
SCALES = [1e-2, 1e-4, 1e-3, 1e-1, 1e-5]          # gradient scale of step 1 ... 5 (times N(0, 1); tables: 1e-3 times these)


def hyper(lr=1e-3, beta_1=0.9, beta_2=0.5, epsilon=1e-7):
    """Keras' hyper-parameters are float32 variables: the reference takes their float32 values, as Python floats."""
    return dict(lr=float(np.float32(lr)), b1=float(np.float32(beta_1)), b2=float(np.float32(beta_2)), eps=float(np.float32(epsilon)))


def amsgrad64(h, p, g, m, v, vhat, t, lr=None):
    """One step in float64; t the 1-based step, lr the step's rate when it is not h["lr"] (a schedule).  Returns (p, m, v, vhat)."""
    lr = h["lr"] if lr is None else lr
    alpha = lr * np.sqrt(1 - h["b2"] ** t) / (1 - h["b1"] ** t)
    m = m + (g - m) * (1 - h["b1"])
    v = v + (g * g - v) * (1 - h["b2"])
    vhat = np.where(vhat < v, v, vhat)
    return p - m * alpha / (np.sqrt(vhat) + h["eps"]), m, v, vhat


def adam64(h, p, g, m, v, t):
    """The same step with vhat ignored (plain Adam): what the rule must NOT be."""
    alpha = h["lr"] * np.sqrt(1 - h["b2"] ** t) / (1 - h["b1"] ** t)
    m = m + (g - m) * (1 - h["b1"])
    v = v + (g * g - v) * (1 - h["b2"])
    return p - m * alpha / (np.sqrt(v) + h["eps"]), m, v


def vhat_next32(vhat_before, v_after):
    """The exact fp32 relation: no rounding in it, so the device's vhat must have these bits given the device's own v."""
    vhat_before, v_after = np.asarray(vhat_before, np.float32), np.asarray(v_after, np.float32)
    return np.where(vhat_before < v_after, v_after, vhat_before)


def nrel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))
