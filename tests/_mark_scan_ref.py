"""NumPy reference of the watermark scan (include/fq3hip.h states the windows), built on tests/_mark_ref.py:
the detector's sums per block of 16 frames, added over each window's block range.  A helper, not a test."""
import numpy as np

import _mark_ref as R

BLOCK = 16


def windows(nb, win, hop):
    """block ranges [(start, end)] of a clip of ``nb`` blocks"""
    if nb <= win:
        return [(0, nb)]
    return [(min(w * hop, nb - win), min(w * hop, nb - win) + win) for w in range(1 + -(-(nb - win) // hop))]


def scan_tables(r, key, win_blocks, hop_blocks, dtype=np.float64):
    """z[W][32][128]"""
    r = np.asarray(r, dtype=dtype)
    T = -(-len(r) // R.H) + 1
    wc, ws = R._tables(dtype)
    c = R.chips(key).astype(dtype)
    rows = (np.arange(1, T - 1)[:, None] + np.arange(R.PERIOD)[None, :]) % R.PERIOD              # [t][phase], t from the clip's start
    spans = windows(-(-(T - 2) // BLOCK), win_blocks, hop_blocks)
    z = np.zeros((len(spans), len(R.OFFSETS), R.PERIOD), dtype=dtype)
    for oi, o in enumerate(R.OFFSETS):
        fr = R._frames(r, int(o), T, dtype)
        re, im = fr @ wc.T, fr @ ws.T
        L = np.log(np.sqrt(re * re + im * im) + dtype(1e-9))
        d = np.clip(L[1:-1] - dtype(0.5) * (L[:-2] + L[2:]), -2, 2).astype(dtype)                # d[i] is frame 1 + i
        for w, (s, e) in enumerate(spans):
            dw = d[BLOCK * s:BLOCK * e]
            en = np.sum(dw * dw)
            if en > 0:
                z[w, oi] = np.einsum("tj,tpj->p", dw, c[rows[BLOCK * s:BLOCK * e]]) / np.sqrt(en)
    return z
