"""``torch.optim.Adam``'s update (no weight decay, no amsgrad) in float64 numpy: the reference of both trainers' tests."""
import numpy as np


def adam_step_f64(w, m, v, g, k, lr, beta1, beta2, eps):
    """One Adam step in float64 numpy on arrays of any shape (step number k = 1, 2, ...) -> (w, m, v)."""
    w, m, v, g = (np.asarray(a, dtype=np.float64) for a in (w, m, v, g))
    m = m + (g - m) * (1.0 - beta1)
    v = beta2 * v + (1.0 - beta2) * g * g
    w = w - (lr / (1.0 - beta1 ** k)) * m / (np.sqrt(v) / np.sqrt(1.0 - beta2 ** k) + eps)
    return w, m, v
