"""The counter generator of rng_mode='device' (csrc/device_common.h) restated in NumPy, from its definitions.

Everything up to the last conversion to float is integer arithmetic modulo 2^32 / 2^64, so the words below are EXACTLY the
kernels' words; a handle in rng_mode='inject' fed these draws must then compute what a handle in rng_mode='device' computes
(tests/test_device_rng_gpu.py), and the draws themselves can be held to what a sound generator gives
(tests/test_device_rng_cpu.py).

What is keyed by what
---------------------
  key(seed, step)            = rng_key(seed, step, 0) = seed ^ step * 0xD1B54A32D192ED03          (64 bit)
  key of stream sid          = key ^ sid * 0xA0761D6478BD642F
  word(seed, step, sid, r, c) = hash_cell(key of stream sid, r, c)                                 (32 bit)

  dropout   stream i of a step is mask i of aae_rng_inject (0-1 enc / 2-3 dec of the reconstruction phase, 4-5 the
            discriminator on [z_real; z_fake], 8-11 enc / disc of the generator phase); cell (r, c) of the GLOBAL batch is
            kept iff word >= min(2^32 - 1, p * 2^32) with p the float32 dropout rate
  prior     stream 100: gauss cell (r, j) from the words of columns 2j and 2j + 1 (Box-Muller on their top 24 bits),
            categorical row r from the word of column 0xFFFFFFFF (class = word mod n_code), bernoulli draws nothing (zeros)
  VAE eps   stream 12, as the gauss prior; r is the row WITHIN THE CALL (include/aaerec_hip.h, aae_vae_step)

The step value
--------------
`step` is what *step_ctr holds once a step is open: a handle's counter starts at 0 and advance_step_body (csrc/kernels.h)
adds one when a training call opens its step (`*ctr += 1`), BEFORE anything of that step is drawn.  So the n-th step of a
fresh handle (n = 1, 2, ...) draws with step value n, forward and backward alike; a call that opens no step (predict,
aae_vae_predict, the rank calls) draws with the count of the steps opened so far (0 on a fresh handle).  A restored
checkpoint restores the counter.

Accuracy of the Gaussian
------------------------
f1 in (0, 1] and f2 in [0, 1) are formed in float32 exactly as the kernels form them (both are exact: 24-bit integers times
2^-24); sqrt(-2 ln f1) cos(2 pi f2) is then evaluated in float64 with the kernels' float32 constant for 2 pi.  The kernels
evaluate it with fp32 logf / cosf / sqrtf: the argument of cosf is rounded to fp32 (up to 2 pi 2^-24 = 3.7e-7 absolute),
times the radius (at most sqrt(48 ln 2) = 5.77), plus a few units in the last place of the result: below 5e-6 in all.
"""
import numpy as np

M64 = (1 << 64) - 1
STEP_MUL = 0xD1B54A32D192ED03
STREAM_MUL = 0xA0761D6478BD642F
PRIOR_STREAM, EPS_STREAM = 100, 12
TWO_PI_F32 = float(np.float32(6.283185307179586))
PRIORS = {"gauss": 0, "categorical": 1, "bernoulli": 2}


def step_value(n, restored=0):
    """The step value of the n-th training step (n = 1, 2, ...) of a handle whose counter was `restored` (0: fresh): the
    counter is advanced when the step opens, before its first draw."""
    return restored + n


def rng_key(seed, step, stream=0):
    """device_common.h rng_key: uint64."""
    return (int(seed) ^ ((int(step) * STEP_MUL) & M64) ^ ((int(stream) << 56) & M64)) & M64


def stream_key(seed, step, sid):
    """The key every dropout / prior / eps stream hashes its cells with."""
    return rng_key(seed, step, 0) ^ ((int(sid) * STREAM_MUL) & M64)


def hash_cell(key, rows, cols):
    """device_common.h hash_cell over the grid rows x cols -> uint32 [len(rows), len(cols)]."""
    lo, hi = np.uint32(key & 0xFFFFFFFF), np.uint32(key >> 32)
    r = (np.asarray(rows, dtype=np.int64) & 0xFFFFFFFF).astype(np.uint32)[:, None]
    c = (np.asarray(cols, dtype=np.int64) & 0xFFFFFFFF).astype(np.uint32)[None, :]
    with np.errstate(over="ignore"):
        x = (lo + r * np.uint32(0x9E3779B1)) ^ (hi + c * np.uint32(0x85EBCA77))
        x ^= x >> np.uint32(16)
        x *= np.uint32(0x7FEB352D)
        x ^= x >> np.uint32(15)
        x *= np.uint32(0x846CA68B)
        x ^= x >> np.uint32(16)
    return x


def words(seed, step, sid, n_rows, n_cols, row0=0):
    """The words of stream sid for global rows [row0, row0 + n_rows) and columns [0, n_cols)."""
    return hash_cell(stream_key(seed, step, sid), np.arange(n_rows, dtype=np.int64) + row0, np.arange(n_cols, dtype=np.int64))


def keep_threshold(p):
    """make_drop (csrc/abi_model.h): uint32(min(2^32 - 1, p * 2^32)) with p the float32 rate; p == 0 disables dropout
    (None: every cell is kept, no word is compared)."""
    p = float(np.float32(p))
    if not p > 0.0:
        return None
    return int(min(4294967295.0, p * 4294967296.0))


def keep(w, p):
    thr = keep_threshold(p)
    if thr is None:
        return np.ones(w.shape, dtype=np.uint8)
    return (w >= np.uint32(thr)).astype(np.uint8)


def dropout_masks(seed, step, p1, p2, B, h, row0=0, global_rows=0):
    """The 12 uint8 keep-masks [B, h] of one step in aae_rng_inject's layout.  Even masks belong to the first hidden layer
    of their network (rate p1), odd ones to the second (p2).  Masks 4 / 6 are the discriminator's first layer on the z_real
    / z_fake rows: rows [0, B) and [B, 2B) of stream 4, which make_drop places at global rows row0 + r (goff_a) and
    row0 + global_rows + r (goff_b; B + r when no global batch is set); 5 / 7 the same of stream 5."""
    fake0 = row0 + (global_rows if global_rows > 0 else B)
    out = []
    for i in range(12):
        p = p1 if i % 2 == 0 else p2
        sid, r0 = (i, row0) if i not in (6, 7) else (i - 2, fake0)
        out.append(keep(words(seed, step, sid, B, h, r0), p))
    return out


def _box_muller(w):
    """w: words [rows, 2n] -> float64 [rows, n]."""
    u1, u2 = w[:, 0::2] >> np.uint32(8), w[:, 1::2] >> np.uint32(8)
    f1 = (u1.astype(np.float32) + np.float32(1.0)) * np.float32(1.0 / 16777216.0)       # (0, 1]
    f2 = u2.astype(np.float32) * np.float32(1.0 / 16777216.0)                           # [0, 1)
    return np.sqrt(-2.0 * np.log(f1.astype(np.float64))) * np.cos(TWO_PI_F32 * f2.astype(np.float64))


def gauss(seed, step, sid, B, c, row0=0):
    return _box_muller(words(seed, step, sid, B, 2 * c, row0))


def categorical_classes(seed, step, B, c, row0=0):
    """The class of every row of the categorical prior."""
    w = hash_cell(stream_key(seed, step, PRIOR_STREAM), np.arange(B, dtype=np.int64) + row0, [0xFFFFFFFF])[:, 0]
    return (w % np.uint32(c)).astype(np.int64)


def prior(seed, step, kind, B, c, scale=1.0, row0=0):
    """z_real [B, c] float32 of a step, times `scale` (the kernels multiply in float32).  Injected draws are handed over
    BEFORE prior_scale: pass scale = 1 for those."""
    k = PRIORS[kind] if isinstance(kind, str) else int(kind)
    if k == 0:
        z = gauss(seed, step, PRIOR_STREAM, B, c, row0).astype(np.float32)
    elif k == 1:
        z = np.zeros((B, c), dtype=np.float32)
        z[np.arange(B), categorical_classes(seed, step, B, c, row0)] = 1.0
    else:
        z = np.zeros((B, c), dtype=np.float32)          # the reference's randint(0, 1) is always 0
    return z * np.float32(scale)


def vae_eps(seed, step, stream, B, c, row0=0):
    """eps [B, c] float32 of reparametrize(): stream 12 in every VAE program."""
    return gauss(seed, step, stream, B, c, row0).astype(np.float32)
