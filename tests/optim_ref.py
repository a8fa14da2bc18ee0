"""The float64 oracle of the optimiser step (wekws_amd/csrc/optim.hip.h), torch's own float32 step on the CPU -- the
reference: clip_grad_norm_ + optim.Adam -- and a Python restatement of csrc/optim_plan.h.

The oracle takes the float32 inputs (p, g, m, v) and the step count, widens them to float64 and performs one step in float64
throughout; the norm is sqrt(math.fsum(g^2)) (a float32's square is exact in float64, fsum adds without rounding until the
end).  The hyper-parameters are the Python floats torch holds."""
from __future__ import annotations

import math

import numpy as np

TILE_FLOATS = 4096          # wekws::kOptimTileFloats
FOLD_SEG = 256              # wekws::kOptimFoldSeg
MAX_ELEMS = 1 << 28         # wekws::kOptimMaxElems
STATE_BYTES = 64            # sizeof(wekws::OptimState)
STATE_DTYPE = np.dtype([("step", "<i8"), ("skipped", "<i8"), ("norm", "<f8"), ("bc1", "<f8"), ("bc2sqrt", "<f8"), ("coef", "<f4"),
                        ("norm_f32", "<f4"), ("apply", "<i4"), ("finite", "<i4"), ("step_size", "<f4"), ("bc2sqrt_f32", "<f4")])


def plan(n):
    """{tile floats, tiles, workspace bytes} of wekws_hip_optim_plan, or None where it refuses."""
    if n < 1 or n > MAX_ELEMS:
        return None
    tiles = (n + TILE_FLOATS - 1) // TILE_FLOATS
    segs = (tiles + FOLD_SEG - 1) // FOLD_SEG if tiles > FOLD_SEG else 0
    return TILE_FLOATS, tiles, ((tiles + segs) * 8 + 15) // 16 * 16


def oracle_step(p, g, m, v, step, lr, betas, eps, weight_decay, max_norm):
    """One step from the state after `step` steps -> dict(norm, coef, p, m, v, bc1, bc2sqrt), float64."""
    p, g, m, v = (np.asarray(a, np.float32).astype(np.float64) for a in (p, g, m, v))
    beta1, beta2 = betas
    norm = math.sqrt(math.fsum((g * g).tolist()))
    coef = 1.0 if max_norm == math.inf else min(1.0, max_norm / (norm + 1e-6))
    t = step + 1
    bc1 = 1.0 - beta1 ** t
    bc2sqrt = math.sqrt(1.0 - beta2 ** t)
    gt = coef * g + weight_decay * p
    m1 = beta1 * m + (1.0 - beta1) * gt
    v1 = beta2 * v + (1.0 - beta2) * gt * gt
    p1 = p - (lr / bc1) * m1 / (np.sqrt(v1) / bc2sqrt + eps)
    return dict(norm=norm, coef=coef, p=p1, m=m1, v=v1, bc1=bc1, bc2sqrt=bc2sqrt)


def torch_step(p, g, m, v, step, lr, betas, eps, weight_decay, max_norm):
    """The reference: clip_grad_norm_ and the single-tensor optim.Adam in float32 on the CPU -> dict(norm, p, m, v), float32."""
    import torch
    param = torch.nn.Parameter(torch.from_numpy(np.array(p, np.float32)))
    param.grad = torch.from_numpy(np.array(g, np.float32))
    opt = torch.optim.Adam([param], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, foreach=False)
    if step > 0:
        opt.state[param] = {"step": torch.tensor(float(step)), "exp_avg": torch.from_numpy(np.array(m, np.float32)),
                            "exp_avg_sq": torch.from_numpy(np.array(v, np.float32))}
    else:
        assert not np.any(m) and not np.any(v), "a first step starts from zero moments"
    if max_norm == math.inf:
        norm = torch.linalg.vector_norm(param.grad)
    else:
        norm = torch.nn.utils.clip_grad_norm_([param], max_norm)
    assert bool(torch.isfinite(norm))
    opt.step()
    st = opt.state[param]
    assert float(st["step"]) == step + 1
    return dict(norm=np.float32(norm.item()), p=param.detach().numpy().copy(), m=st["exp_avg"].numpy().copy(),
                v=st["exp_avg_sq"].numpy().copy())
