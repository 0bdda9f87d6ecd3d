"""float64 reference of the voice library search (csrc/voices_kernels.cuh: voices_add_kernel, voices_query_pack_kernel,
voices_scan_kernel, voices_merge_kernel) and the inputs of tests/test_gpu_voices.py.

The bound.  u = 2^-24.  Each side is scaled to unit length in fp32: the sum of squares is D / 256 chained fmas per lane, two adds
and a six-step tree, a relative error of at most (D / 256 + 8) u, halved by the square root; the square root, the reciprocal and the
product with the element round once each: every stored element is within (D / 512 + 7) u of the exact unit vector's, relatively.
The cosine is a chain of D fp32 accumulations of products of those elements: at most D u sum |a_d b_d| <= D u by Cauchy-Schwarz.
To first order |cos - cos64| <= (D + 2 (D / 512 + 7)) u, rounded up here to (D + D / 256 + 16) u: 6.2e-5 at D = 1024."""
import numpy as np


def bound(dim):
    return (dim + dim / 256 + 16) * 2.0 ** -24


def cosines(lib, q):
    """[queries][N] in float64 of float32 inputs; a zero vector gives 0"""
    unit = lambda x: x / np.where(np.linalg.norm(x, axis=1, keepdims=True) > 0, np.linalg.norm(x, axis=1, keepdims=True), 1.0)
    return unit(np.asarray(q, np.float64)) @ unit(np.asarray(lib, np.float64)).T


def top_k(lib, q, k, dead=()):
    """(idx int[queries][k], cos float64[queries][k]) ordered by (cosine descending, index ascending); missing slots -1 / -2"""
    c = cosines(lib, q)
    alive = np.array([i for i in range(len(lib)) if i not in set(dead)], dtype=np.int64)
    idx, cos = np.full((len(q), k), -1, np.int64), np.full((len(q), k), -2.0)
    for r in range(len(q)):
        order = alive[np.lexsort((alive, -c[r, alive]))][:k]
        idx[r, :len(order)], cos[r, :len(order)] = order, c[r, order]
    return idx, cos


def ladder(dim, n, n_queries, seed):
    """A library [n][dim] and queries whose every rank is decided.  u, v, w: orthogonal directions (u, v dense in every coordinate).
    Query i sits at angle 0.005 i in the (u, v) plane; 16 ladder rows (fewer when n < 16) at angles 0.3 + 0.1 j, at seeded places of
    the library, and every other row at an angle in [2.2, 3.0]: neighbouring ladder cosines differ by more than 1e-2 for every query
    and the others lie far below the last.  Every row carries a component along w (0.2 or 0.5 of its length) and its own scale."""
    rng = np.random.default_rng(seed)
    basis, _ = np.linalg.qr(rng.standard_normal((dim, 3)))
    u, v, w = basis.T
    at = lambda phi, side: np.outer(np.cos(phi), u) + np.outer(np.sin(phi), v) + np.outer(side, w)
    lib = at(rng.uniform(2.2, 3.0, n), np.full(n, 0.5) * rng.choice([-1.0, 1.0], n))
    steps = min(n, 16)
    places = rng.permutation(n)[:steps]
    lib[places] = at(0.3 + 0.1 * rng.permutation(steps), np.full(steps, 0.2))
    lib *= rng.uniform(0.5, 20.0, (n, 1))
    q = at(0.005 * np.arange(n_queries), np.zeros(n_queries)) * rng.uniform(0.5, 20.0, (n_queries, 1))
    return lib.astype(np.float32), q.astype(np.float32)
