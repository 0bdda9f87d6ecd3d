"""NumPy implementation of the seeded-noise contract (csrc/noise_kernels.cuh): Philox4x32-10 on uint64 arrays,
then the variate transform.  The reference of tests/test_noise_reference_cpu.py and tests/test_gpu_noise.py.

``philox`` takes keyword switches that each break the contract in one way (the mutants of the CPU test); the defaults are the contract.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
FIRST_SLOT = 0xFFFFFFFF


def philox(c0, c1, c2, c3, k0, k1, rounds=10, swap_multipliers=False, bump_key=True):
    """Philox4x32 on arrays (or scalars) of counters and keys -> four uint32 arrays."""
    c = [np.asarray(x, dtype=np.uint64) & MASK for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    m0, m1 = (np.uint64(M1), np.uint64(M0)) if swap_multipliers else (np.uint64(M0), np.uint64(M1))
    sh = np.uint64(32)
    for _ in range(rounds):
        p0, p1 = m0 * c[0], m1 * c[2]                       # 32 x 32 -> 64 bits: exact in uint64
        c = [(p1 >> sh) ^ c[1] ^ k0, p1 & MASK, (p0 >> sh) ^ c[3] ^ k1, p0 & MASK]
        if bump_key:
            k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return [x.astype(np.uint32) for x in c]


def words(seed, frame, slot, V, v_swapped=False, slot_frame_swapped=False, **mutant):
    """The raw words of one row: uint32[V]."""
    seed = int(seed)
    v = np.arange(int(V), dtype=np.uint64)
    ctr, lane = (v & np.uint64(3), v >> np.uint64(2)) if v_swapped else (v >> np.uint64(2), v & np.uint64(3))
    c1, c2 = (slot, frame) if slot_frame_swapped else (frame, slot)
    out = philox(ctr, np.uint64(int(c1) & 0xFFFFFFFF), np.uint64(int(c2) & 0xFFFFFFFF), np.uint64(0),
                 seed & 0xFFFFFFFF, seed >> 32, **mutant)
    return np.choose(lane.astype(np.int64), out).astype(np.uint32)


def variates(w, shift=9):
    """words -> fp32 Exp(1) variates: k = w >> 9, u = (2 k + 1) 2^-24, -ln(u) in fp64, one rounding to fp32."""
    k = (np.asarray(w, dtype=np.uint32) >> np.uint32(shift)).astype(np.float64)
    u = (2.0 * k + 1.0) * 2.0 ** -(33 - shift)
    return (-np.log(u)).astype(np.float32)


def to_bf16_bits(x32):
    """fp32 -> bf16 bit patterns (uint16), round to nearest even (finite inputs)."""
    b = np.asarray(x32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    b = b + np.uint64(0x7FFF) + ((b >> np.uint64(16)) & np.uint64(1))
    return (b >> np.uint64(16)).astype(np.uint16)


def bf16_bits_to_f32(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def row(seed, frame, slot, V, **mutant):
    """One noise row in fp32."""
    shift = mutant.pop("shift", 9)
    return variates(words(seed, frame, slot, V, **mutant), shift=shift)


def talker_row(seed, frame, V):
    return row(seed, frame, 0, V)


def pred_rows(seed, frame, G1, Vp):
    """[G - 1][Vp]: predictor codebook cb uses slot 1 + cb."""
    return np.stack([row(seed, frame, 1 + cb, Vp) for cb in range(G1)])


def first_row(seed, V):
    return row(seed, 0, FIRST_SLOT, V)
