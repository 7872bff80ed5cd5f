"""float64 reference of the weight EMA that mmbert_adamw_ema keeps (no GPU): one update, and the bound the kernel is held to."""
import numpy as np
import torch


def ema_step(E0, P, omd):
    """E0 + omd (P - E0) in float64: the average after the parameters became P; omd = 1 - decay."""
    E0, P = torch.as_tensor(E0).double(), torch.as_tensor(P).double()
    return E0 + float(omd) * (P - E0)


def omd_f32(decay):
    """1 - decay formed in double and rounded to fp32 once, as a float64 value: what the kernel multiplies by."""
    return float(np.float32(1.0 - float(decay)))


def ema_bound(E0, P, omd):
    """|got - ref| allowed of the fp32 kernel: 5e-7 (|E0| + omd |P|) + 1e-30, the project's fp32-roundings-only bound of the AdamW
    moments.  Either algebraic form of the lerp -- e + omd (p - e) or (1 - omd) e + omd p -- makes three fp32 roundings, each at most
    2^-24 = 6e-8 of a term no larger than that scale: 1.8e-7 in all."""
    E0, P = torch.as_tensor(E0).double(), torch.as_tensor(P).double()
    return 5e-7 * (E0.abs() + float(omd) * P.abs()) + 1e-30
