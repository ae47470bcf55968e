"""Float64 restatement of the optimizer update of csrc/k_train.hip (k_train_adamw / k_train_adamw_dev): torch.optim.AdamW with amsgrad off - decoupled
weight decay, then p -= lr / (1 - b1^t) . m / (sqrt(v) / sqrt(1 - b2^t) + eps) - as written in the comment above k_train_adamw.  Plain numpy, no torch call in
the arithmetic; tests/test_train_ref_cpu.py pins it to torch's own float64 update, tests/test_gpu_train_graph.py holds the kernels to it."""
import math

import numpy as np


def adamw_scalars(t, lr, betas):
    """(lr / (1 - b1^t), 1 / sqrt(1 - b2^t)) in double: the two values k_train_adamw_scalars leaves in scal[0..1] (there rounded to float32)."""
    b1, b2 = (float(b) for b in betas)
    return float(lr) / (1.0 - b1 ** int(t)), 1.0 / math.sqrt(1.0 - b2 ** int(t))


def adamw_ref(p, g, m, v, t, lr, betas, eps, weight_decay):
    """One AdamW step, the t-th (1-based), on float64 arrays -> (p, m, v), new arrays; the inputs are left alone."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    b1, b2 = (float(b) for b in betas)
    step_size, rbc2 = adamw_scalars(t, lr, betas)
    m = m + (g - m) * (1.0 - b1)
    v = b2 * v + (1.0 - b2) * g * g
    p = p * (1.0 - float(lr) * float(weight_decay)) - step_size * (m / (np.sqrt(v) * rbc2 + float(eps)))
    return p, m, v
