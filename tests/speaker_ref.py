"""Float64 reference of a blended voice: row[c] = sum_k w_k * table[id_k][c], and the bound the fp32
kernel is held to."""
import numpy as np


def blend(table, ids, weights):
    """table [n, gin], K ids, K weights -> the row [gin] in float64 (the weights as given: pass the fp32 values that
    were actually sent)."""
    table = np.asarray(table, dtype=np.float64)
    ids = [int(i) for i in ids]
    w = np.asarray(list(weights), dtype=np.float64)
    assert len(ids) == w.size >= 1
    return (w[:, None] * table[ids]).sum(axis=0)


def bound(table, ids, weights):
    """K * 2^-23 * sum_k |w_k * e_k[c]| per channel: what a K-term fp32 chain (one rounded product, K - 1 fused
    multiply-adds, each within half an ulp = 2^-24 relative of a partial sum that never exceeds sum_k |w_k e_k| (1 +
    K 2^-24)) stays inside with a factor two to spare.  Derived, not measured."""
    table = np.asarray(table, dtype=np.float64)
    ids = [int(i) for i in ids]
    w = np.asarray(list(weights), dtype=np.float64)
    return len(ids) * 2.0 ** -23 * np.abs(w[:, None] * table[ids]).sum(axis=0)
