"""`utils.unmap.unmap` (reference: lib/utils/unmap.py:11-22): values of a subset put back at their places in the full set."""
import numpy as np


def unmap(data, count, inds, fill=0):
    """data [len(inds), ...] -> float32 [count, ...]: `fill` everywhere, data at rows `inds`."""
    out = np.full((count,) + data.shape[1:], fill, dtype=np.float32)
    out[inds] = data
    return out
