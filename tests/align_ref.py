"""NumPy restatements for the forced alignment (`net.align`): Monotonic Alignment Search after
monotonic_align/core.pyx:7-37 line by line, the negative cross-entropy matrix of models.py:670-675 in float64, a
brute-force maximum over all monotone paths, and the whole chain (enc_p, enc_q, forward flow, neg_cent, search)
from `oracle.ref_infer` in float64."""
import itertools
import math

import numpy as np

MAX_NEG_VAL = -1e9


def maximum_path_each(value, t_y, t_x, dtype=np.float32):
    """core.pyx:7-37 on a copy of value [T_t, T_s]: -> (path int32 [T_t, T_s], cumulated value).
    dtype np.float32 = the reference's arithmetic, np.float64 = the yardstick.  t_x <= t_y required (the
    reference reads outside its arrays otherwise)."""
    assert 1 <= t_x <= t_y <= value.shape[0] and t_x <= value.shape[1]
    value = np.array(value, dtype=dtype)            # the reference cumulates in place
    path = np.zeros(value.shape, np.int32)
    neg = dtype(MAX_NEG_VAL)
    zero = dtype(0.)
    for y in range(t_y):
        for x in range(max(0, t_x + y - t_y), min(t_x, y + 1)):
            if x == y:
                v_cur = neg
            else:
                v_cur = value[y - 1, x]
            if x == 0:
                if y == 0:
                    v_prev = zero
                else:
                    v_prev = neg
            else:
                v_prev = value[y - 1, x - 1]
            value[y, x] = dtype(value[y, x] + (v_cur if v_cur > v_prev else v_prev))    # C's max(v_prev, v_cur)
    index = t_x - 1
    for y in range(t_y - 1, -1, -1):
        path[y, index] = 1
        if index != 0 and (index == y or value[y - 1, index] < value[y - 1, index - 1]):
            index = index - 1
    return path, value


def maximum_path(values, t_ys, t_xs, dtype=np.float32):
    """maximum_path_c over a batch [B, T_t, T_s] -> (paths int32 [B, T_t, T_s], w int32 [B, T_s])."""
    values = np.asarray(values)
    paths = np.zeros(values.shape, np.int32)
    for b in range(values.shape[0]):
        paths[b] = maximum_path_each(values[b], int(t_ys[b]), int(t_xs[b]), dtype)[0]
    return paths, paths.sum(1).astype(np.int32)


def neg_cent(z_p, m_p, logs_p):
    """models.py:670-675 in float64.  z_p [B, I, T_t], m_p / logs_p [B, I, T_s] ->
    (value [B, T_t, T_s], sum of |summands| per cell: the 4 I terms the value is the sum of)."""
    z = np.asarray(z_p, np.float64)
    m = np.asarray(m_p, np.float64)
    lg = np.asarray(logs_p, np.float64)
    s = np.exp(-2.0 * lg)
    c1 = -0.5 * math.log(2 * math.pi) - lg                    # [B, I, T_s]
    c4 = -0.5 * m * m * s
    zt = z.transpose(0, 2, 1)                                  # [B, T_t, I]
    n2 = np.matmul(-0.5 * zt * zt, s)
    n3 = np.matmul(zt, m * s)
    value = c1.sum(1)[:, None, :] + n2 + n3 + c4.sum(1)[:, None, :]
    mag = (np.abs(c1).sum(1) + np.abs(c4).sum(1))[:, None, :] + np.matmul(0.5 * zt * zt, s) + np.matmul(np.abs(zt), np.abs(m) * s)
    return value, mag


def exp_term_mag(z_p, m_p, logs_p):
    """Sum over d of the |summands| that carry the factor e^{-2 logs_p} (terms 2, 3 and 4), per cell."""
    z = np.asarray(z_p, np.float64)
    m = np.asarray(m_p, np.float64)
    s = np.exp(-2.0 * np.asarray(logs_p, np.float64))
    zt = z.transpose(0, 2, 1)
    return np.matmul(0.5 * zt * zt, s) + np.matmul(np.abs(zt), np.abs(m) * s) + (0.5 * m * m * s).sum(1)[:, None, :]


def generate_path(w, t_y):
    """commons.py:128-143 for one utterance: durations w [t_x] -> path [t_y, t_x]."""
    w = np.asarray(w, np.int64)
    cum = np.cumsum(w)
    y = np.arange(t_y)[:, None]
    return ((y < cum[None, :]) & (y >= (cum - w)[None, :])).astype(np.int32)


def path_score(value, path):
    return float(np.sum(np.asarray(value, np.float64) * path))


def all_monotone_paths(t_y, t_x):
    """Every path with one token per frame, tokens in order, at least one frame per token: as durations."""
    for cuts in itertools.combinations(range(1, t_y), t_x - 1):
        edges = (0,) + cuts + (t_y,)
        yield np.diff(edges)


def brute_force(value, t_y, t_x):
    """max over all monotone paths of the float64 score -> (best score, durations of one maximiser)."""
    best, arg = -np.inf, None
    for w in all_monotone_paths(t_y, t_x):
        sc = path_score(value[:t_y, :t_x], generate_path(w, t_y))
        if sc > best:
            best, arg = sc, w
    return best, arg


def chain(sd, cfg, x, x_lengths, y, y_lengths, sid=None, noise=None, noise_scale=1.0, dtype="float64"):
    """The body of SynthesizerTrn.forward up to models.py:680 from the oracle's stages, in `dtype`:
    -> dict(m_text, logs_text, z, z_p, neg_cent, mag) as NumPy arrays."""
    import torch
    from oracle import ref_infer as R
    td = getattr(torch, dtype)
    W = R.Weights(sd)
    W.sd = {k: v.to(td) for k, v in W.sd.items()}
    with torch.no_grad():
        ids = torch.as_tensor(np.asarray(x)).long()
        xl = torch.as_tensor(np.asarray(x_lengths)).long()
        _, m_p, logs_p, _ = R.text_encoder(W, cfg, ids, xl)
        g = None
        if sid is not None:
            g = W["emb_g.weight"][torch.as_tensor(np.asarray(sid)).long()].unsqueeze(-1)
        nz = None
        if noise is not None and float(noise_scale) != 0.0:
            nz = torch.as_tensor(np.asarray(noise)).to(td) * float(noise_scale)
        z, _, _, y_mask = R.posterior_encoder(W, cfg, torch.as_tensor(np.asarray(y)).to(td),
                                              torch.as_tensor(np.asarray(y_lengths)).long(), g, nz)
        z_p = R.flow_forward(W, cfg, z, y_mask, g)
    v, mag = neg_cent(z_p.numpy(), m_p.numpy(), logs_p.numpy())
    return dict(m_text=m_p.numpy(), logs_text=logs_p.numpy(), z=z.numpy(), z_p=z_p.numpy(), neg_cent=v, mag=mag)
