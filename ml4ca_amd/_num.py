"""Host arithmetic shared by the host statements of the device laws (train.adam_step_ref, deploy.BatchedNNAllocator)."""
import numpy as np


def _fma32(a, b, c):
    """fmaf on float32 operands, correctly rounded: the product is exact in float64, the sum is rounded to ODD there (TwoSum gives the
    rounding error), and a round-to-odd float64 rounds to float32 as the exact value would."""
    a, b, c = (np.asarray(x, np.float32).astype(np.float64) for x in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    s = np.atleast_1d(s).copy()
    err = np.broadcast_to(np.atleast_1d(err), s.shape)
    fix = (err != 0) & ((s.view(np.int64) & 1) == 0) & np.isfinite(s)
    s[fix] = np.nextafter(s[fix], np.where(err[fix] > 0, np.inf, -np.inf))
    return s.astype(np.float32)
