"""References, bounds and schedules for the deferred first-layer Adam (csrc/kernels.h: lazy_replay, w1_catchup_kernel,
advance_step_body) - no GPU needed.

A row of enc.lin1 whose item only ever enters a batch with VALUE 0 gets a gradient of exactly 0 on every path, so its
(p, m1, v1, m3, v3) follow zero-gradient Adam: a function of the row's own state, the step numbers and the two learning
rates.  Per step t, enc_optim (moments m1 / v1, rate lr_gen) then gen_optim (m3 / v3, lr_reg):

    m <- m - b1c * m;  v <- b2 * v;  p <- p - lr(t) / bc1(t) * m / (sqrt(v) / sqrt(bc2(t)) + eps)

with b1c = float32(0.1), b2 = float32(0.999), eps = float32(1e-8) (the constants torch's fp32 Adam and adam_update use),
bc1 = 1 - 0.9^t, bc2 = 1 - 0.999^t.

A row is brought up to date in LAZY SEGMENTS.  `touches` is the sorted list of steps THROUGH which a catch-up brought the
row ("sync points"); a training step t that holds the item is the two sync points t - 1 (the catch-up in front of the
gather) and t (the step's own update: a segment of one step, the same arithmetic).  Of a segment longer than kLazyReplay =
128 steps the device applies the first 128 parameter increments and drops the rest; the moments decay over the whole
segment (closed form beyond the 128th step).

    replay64   the float64 reference (with the documented truncation) and the dropped tail
    replay32   a float32 restatement of lazy_replay on a 65 536-slot ring written as advance_step_body writes it
    bounds     the tolerances on |device - replay64|, derived below from u = 2^-24
    Plan       one run's schedule (touches, learning rates, reloads of probe moments) shared by the CPU and GPU tests
"""
import math

import numpy as np

U = 2.0 ** -24                       # unit roundoff of fp32; one ulp <= 2 U relative
K_REPLAY = 128                       # kLazyReplay
CAP = 65536                          # kLazyTabCap
B1C = float(np.float32(0.1))
B2 = float(np.float32(0.999))
EPS = float(np.float32(1e-8))
C_M = np.float32(-0.15200309344504997)       # log2(0.9)   (lazy_replay's two constants)
C_V = np.float32(-0.0014434168696687186)     # log2(0.999)
FLOOR = 1e-37                        # absolute floor for moments that underflow
KEYS = ("p", "m1", "v1", "m3", "v3")


def step_scalars(t, lr_gen, lr_reg):
    """(lr_gen / bc1, lr_reg / bc1, 1 / sqrt(bc2)) of step t in float64 - what advance_step_body rounds to fp32."""
    bc1, bc2 = 1.0 - 0.9 ** t, 1.0 - 0.999 ** t
    return lr_gen / bc1, lr_reg / bc1, 1.0 / math.sqrt(bc2)


def _segments(t0, touches, t_end):
    pts = sorted({int(t) for t in touches if t0 < t < t_end} | {int(t_end)})
    a = int(t0)
    for b in pts:
        yield a, b
        a = b


def _walk(state, t0, touches, t_end, lr_gen_of, lr_reg_of):
    """The float64 trajectory and, along it, the error budget of an fp32 device that follows lazy_replay.

    Budget, in units of u = 2^-24 (1 ulp <= 2 u):
    * moments, replayed step:  m <- m + 0.1f (0 - m) is two roundings, v <- v 0.999f one: the relative error of each grows
      by at most 2 u per replayed step (the replayed part of a segment: <= 2 * 128 u).
    * moments, closed form over `rest` steps:  d = exp2f((float) rest * c) against the reference's b^rest.
        - the argument: c is an fp32 constant and the product is rounded: |rest c| * 2 u absolute, * ln 2 relative in d;
        - exp2f: 1 ulp (2 u), the conversion of rest and the final product m * d: 3 u;   together 5 u
        - the kernel's constants are the exact powers 0.9^rest / 0.999^rest, the reference's are the fp32 constants'
          powers: rest * |float32(0.999) - 0.999| / 0.999 for v and rest * |(1 - float32(0.1)) - 0.9| / 0.9 for m (eight
          times smaller).  This term is no rounding: kernel and
          restatement attain it in full, so it is also handed out on its own (tol['systematic']).
    * p, per replayed update (two per step):
        - the rounding of the sum: u |p|;
        - the increment (nss * m) * rcp(sqrt(v) * ibc2 + eps), relative: two products and the sum of the denominator 1 u
          each, the product by ibc2 1 u, sqrtf and rcpf 1 ulp = 2 u each, the two table entries rounded to fp32 1 u each
          (10 u), plus the accumulated relative error of m and of sqrt(v) (half of v's).
    """
    x = {k: np.array(state[k], dtype=np.float64) for k in KEYS}
    p, m1, v1, m3, v3 = (x[k] for k in KEYS)
    tail = np.zeros_like(p)
    tol_p = np.zeros_like(p)
    em = ev = 0.0                      # accumulated relative error budget of the moments (both sets take the same steps)
    sm = sv = 0.0                      # ... of which the constants' mismatch: systematic, attained in full
    for a, b in _segments(t0, touches, t_end):
        n = b - a
        nl = min(n, K_REPLAY)
        for j in range(1, n + 1):
            t = a + j
            sg, sr, ib = step_scalars(t, lr_gen_of(t), lr_reg_of(t))
            m1 = m1 - B1C * m1
            v1 = B2 * v1
            d1 = -sg * m1 / (np.sqrt(v1) * ib + EPS)
            m3 = m3 - B1C * m3
            v3 = B2 * v3
            d3 = -sr * m3 / (np.sqrt(v3) * ib + EPS)
            if j <= nl:
                em += 2 * U
                ev += 2 * U
                rel = 10 * U + em + 0.5 * ev
                p = p + d1
                tol_p += np.abs(d1) * rel + U * np.abs(p)
                p = p + d3
                tol_p += np.abs(d3) * rel + U * np.abs(p)
            else:
                tail += np.abs(d1) + np.abs(d3)
        rest = n - nl
        if rest > 0:
            sm += rest * abs((1.0 - B1C) - 0.9) / 0.9
            sv += rest * abs(B2 - 0.999) / 0.999
            em += abs(rest * float(C_M)) * math.log(2.0) * 2 * U + 5 * U + rest * abs((1.0 - B1C) - 0.9) / 0.9
            ev += abs(rest * float(C_V)) * math.log(2.0) * 2 * U + 5 * U + rest * abs(B2 - 0.999) / 0.999
    out = dict(p=p, m1=m1, v1=v1, m3=m3, v3=v3)
    tol = dict(p=tol_p, m1=np.abs(m1) * em + FLOOR, m3=np.abs(m3) * em + FLOOR,
               v1=np.abs(v1) * ev + FLOOR, v3=np.abs(v3) * ev + FLOOR)
    # (the part of each bound that the constants' mismatch takes: the kernel - and replay32 - attain it in full)
    tol["systematic"] = dict(p=np.zeros_like(p), m1=np.abs(m1) * sm, m3=np.abs(m3) * sm, v1=np.abs(v1) * sv, v3=np.abs(v3) * sv)
    return out, tail, tol


def replay64(state, t0, touches, t_end, lr_gen_of, lr_reg_of):
    """state: {'p','m1','v1','m3','v3'} arrays of one row (or of rows that share `touches`) as of step t0.
    -> (state as of step t_end, in float64; the sum of the dropped |increments|, per element)."""
    out, tail, _ = _walk(state, t0, touches, t_end, lr_gen_of, lr_reg_of)
    return out, tail


def bounds(state, t0, touches, t_end, lr_gen_of, lr_reg_of):
    """Per element and quantity: the bound on |device - replay64| (derived in _walk's docstring; not fitted)."""
    return _walk(state, t0, touches, t_end, lr_gen_of, lr_reg_of)[2]


class StepTable:
    """LazyTab in its 65 536-slot ring: advance(t) writes the entry of step t AND, one step early, of step t + 1 with the
    rates in force at step t - as advance_step_body does.  `by` records the step whose entry a slot holds."""

    def __init__(self):
        self.nss_gen = np.zeros(CAP, dtype=np.float32)
        self.nss_reg = np.zeros(CAP, dtype=np.float32)
        self.ibc2 = np.zeros(CAP, dtype=np.float32)
        self.by = np.full(CAP, -1, dtype=np.int64)

    def advance(self, t, lr_gen, lr_reg):
        for tt in (t, t + 1):
            sg, sr, ib = step_scalars(tt, lr_gen, lr_reg)
            s = tt & (CAP - 1)
            self.nss_gen[s], self.nss_reg[s], self.ibc2[s] = np.float32(-sg), np.float32(-sr), np.float32(ib)
            self.by[s] = tt


def replay32(state, t0, touches, t_end, lr_gen_of, lr_reg_of, shift=0, reads=None):
    """lazy_replay in NumPy float32: the same operations in the same order (exact sqrt and division for sqrtf / rcpf),
    exp2 of (float) rest * c for the closed form, the per-step scalars from a StepTable filled step by step.
    shift: added to the table index t0 + 1 + j (a deliberately wrong index for the tests).
    reads: a list that receives (step wanted, step whose entry the slot held) for every table read."""
    f = np.float32
    p, m1, v1, m3, v3 = (np.array(state[k], dtype=np.float32) for k in KEYS)
    tab = StepTable()
    segs = {b: a for a, b in _segments(t0, touches, t_end)}
    c01, c999, ceps, zero = f(0.1), f(0.999), f(1e-8), f(0.0)
    for t in range(int(t0) + 1, int(t_end) + 1):
        tab.advance(t, lr_gen_of(t), lr_reg_of(t))
        if t not in segs:
            continue
        a = segs[t]                     # the catch-up through step t runs once step t's entry is in the table
        n = t - a
        nl = min(n, K_REPLAY)
        for j in range(nl):
            s = (a + 1 + j + shift) & (CAP - 1)
            if reads is not None:
                reads.append((a + 1 + j, int(tab.by[s])))
            ng, nr, ib = tab.nss_gen[s], tab.nss_reg[s], tab.ibc2[s]
            m1 = m1 + c01 * (zero - m1)
            v1 = v1 * c999
            p = p + (ng * m1) * (f(1.0) / (np.sqrt(v1) * ib + ceps))
            m3 = m3 + c01 * (zero - m3)
            v3 = v3 * c999
            p = p + (nr * m3) * (f(1.0) / (np.sqrt(v3) * ib + ceps))
        rest = n - nl
        if rest > 0:
            dm = np.exp2(f(rest) * C_M, dtype=np.float32)
            dv = np.exp2(f(rest) * C_V, dtype=np.float32)
            m1, m3, v1, v3 = m1 * dm, m3 * dm, v1 * dv, v3 * dv
    return dict(p=p, m1=m1, v1=v1, m3=m3, v3=v3)


# ---------------------------------------------------------------------------------------------------------------------
# probe states
# ---------------------------------------------------------------------------------------------------------------------
def probe_states(rows, h=12):
    """Deterministic [rows, h] states.  Twelve column kinds, repeated along h (so a column beyond 256 holds one too):
    0-7  the worst ratio a zero-gradient row can reach, m = 0.1 g, v = 0.001 g^2 (|m| / sqrt(v) = 3.16), both signs,
         |g| = 1e-6, 1e-3, 1, 1e2 (times 1, 0.5 or 2 by row);
    8    m = 0 with v > 0;   9  m = v = 0;   10  v so small that eps dominates the denominator;   11  a moderate ratio.
    The gen_optim set (m3, v3) holds the same kinds five columns on.  p in [-0.25, 0.25], a third of them 0."""
    m = np.zeros((rows, h), dtype=np.float64)
    v = np.zeros((rows, h), dtype=np.float64)
    for r in range(rows):
        sc = (1.0, 0.5, 2.0)[r % 3]
        for c in range(h):
            k = c % 12
            if k < 8:
                g = (1e-6, 1e-3, 1.0, 1e2)[k // 2] * sc * (1.0 if k % 2 == 0 else -1.0)
                m[r, c], v[r, c] = 0.1 * g, 0.001 * g * g
            elif k == 8:
                m[r, c], v[r, c] = 0.0, 1e-4 * sc
            elif k == 9:
                m[r, c], v[r, c] = 0.0, 0.0
            elif k == 10:
                m[r, c], v[r, c] = 1e-9 * sc, 1e-24
            else:
                m[r, c], v[r, c] = -0.02 * sc, 3e-3
    rr, cc = np.meshgrid(np.arange(rows), np.arange(h), indexing="ij")
    p = ((rr * 7 + cc * 3) % 11 - 5) * 0.05 * ((rr + cc) % 3 != 0)      # (a p of 0 has no rounding of its own to hide behind)
    f = np.float32
    return dict(p=p.astype(f), m1=m.astype(f), v1=v.astype(f), m3=np.roll(m, 5, axis=1).astype(f),
                v3=np.roll(v, 5, axis=1).astype(f))


def worst_ratio_columns(h=12):
    return np.array([c for c in range(h) if c % 12 < 8])


# ---------------------------------------------------------------------------------------------------------------------
# one run's schedule
# ---------------------------------------------------------------------------------------------------------------------
BASE_LR = (2e-3, 1e-3)
WRAP = CAP - 140                      # a start step from which a 300-step run crosses the ring's wrap in mid-run
START_STEPS = (0, WRAP, 2 * CAP - 5, 20_000_000)


class Plan:
    """The schedule of one run of S steps from step T0, in steps RELATIVE to T0 (step s is step number T0 + s).

    groups: one (reload, gap) per probe row.  reload = 0: the row carries its probe moments from step T0; reload = r > 0:
    it holds zero moments (p does not move) until probe moments are written into it after step r.  Such a RELOAD reads and
    writes the whole moment tensors through the checkpoint entry points, which flush every row: a sync point for all rows,
    from which the gaps are counted.  gap: the row's item first enters a training batch `gap` steps after that (and once more
    18 steps later for gaps up to 3, else 10 steps later, unless again=False); None: never (the final flush only);
    'predict': only an eval-mode predict() reads it, PREDICT_GAP steps after (where the run does not predict: never).
    lr: {s: (gen, reg)} - set_lr in front of step s (all rates, the initial BASE_LR included, times lr_scale).  dense_at: a dense noisy-input step (every row is read: a sync point in
    front of it and one behind it for all rows); it needs the plain autoencoder (ae_only: no gen_optim, m3 = v3 = 0).

    Why reloads: a zero-gradient row's first moment decays by 0.9 per step and nothing renews it, so a learning-rate change
    sixty steps after the moments were loaded moves p by less than the rounding p has accumulated by then - it could be
    ignored unnoticed.  Plan.main therefore reloads twice, and every change falls within a few steps of fresh moments.
    """
    PREDICT_GAP = 135

    def __init__(self, T0, S, groups, lr, predict=False, dense_at=None, h=12, again=True, ae_only=False, lr_scale=1.0):
        self.T0, self.S, self.h = int(T0), int(S), h
        self.base = (BASE_LR[0] * lr_scale, BASE_LR[1] * lr_scale)      # the rates the model is created with
        self.predict, self.dense_at = predict, dense_at
        self.groups = list(groups)
        self.P = len(self.groups)
        self.states = probe_states(self.P, h)
        if ae_only:                     # the plain autoencoder has no gen_optim: its moments stay 0
            self.states["m3"][:] = 0
            self.states["v3"][:] = 0
        self.reloads = sorted({r for r, _ in self.groups if r})
        self.lr = {s: (g * lr_scale, r * lr_scale) for s, (g, r) in lr.items()}
        self.train = [[] for _ in range(self.P)]       # training touches per row
        self.pred_after = {}                           # step -> rows an eval-mode predict reads after it
        for i, (r0, gap) in enumerate(self.groups):
            if gap == "predict":
                if predict:
                    self.pred_after.setdefault(r0 + self.PREDICT_GAP, []).append(i)
            elif gap is not None:
                first = r0 + gap
                cand = (first, first + (18 if gap <= 3 else 10)) if again else (first,)
                self.train[i] = [s for s in cand if s <= self.S]

    @classmethod
    def main(cls, T0, **kw):
        """300 steps.  lr: 5 both x10, 20 gen x0.1, 40 both 0, 60 back, and - about ten steps after the touches of the
        last group's short-gap rows - 68 both x10, 72 back.  Rows: from T0 gaps 1, 2, 3, 30 and never; reloaded after 35:
        gaps 1, 3 and one left to the next reload; reloaded after 56: gaps 1, 2, 3 (their second touch closes a short lazy
        segment over the changes at 68 and 72), 127, 128, 129, 130, 200, never (a final segment of 244) and predict-only."""
        lr = {5: (2e-2, 1e-2), 20: (2e-3, 1e-2), 40: (0.0, 0.0), 60: BASE_LR, 68: (2e-2, 1e-2), 72: BASE_LR}
        groups = [(0, g) for g in (1, 2, 3, 30, None)] + [(35, g) for g in (1, 3, None)] + \
                 [(56, g) for g in (1, 2, 3, 127, 128, 129, 130, 200, None, "predict")]
        return cls(T0, 300, groups, lr, **kw)

    @classmethod
    def long(cls, T0, S, touch):
        """S steps; one row touched once at `touch`, one never: closed-form decays over more than a thousand steps."""
        lr = {5: (2e-2, 1e-2), 20: (2e-3, 1e-2), 40: (0.0, 0.0), 60: BASE_LR}
        return cls(T0, S, [(0, touch), (0, None)], lr, again=False)

    @classmethod
    def cut(cls, T0):
        """140 steps at rate 0 until both rates are set in front of step 128: of a segment that starts at T0 the 128th
        increment - the last one the replay keeps - is then the FIRST that moves p, and nothing hides it (at a constant
        rate it is 1.5e-6 of what p has moved by then, a tenth of p's accumulated rounding).  Rows: never (140 steps: 128
        replayed), first touched at 128, 129 (a segment of exactly 128) and 130 (129: the increment of step 129 dropped)."""
        return cls(T0, 140, [(0, None), (0, 128), (0, 129), (0, 130)], {1: (0.0, 0.0), 128: (2e-2, 1e-2)}, again=False)

    # -- the schedule by step number -------------------------------------------------------------------------------
    def rates(self, s):
        """(gen, reg) in force at relative step s."""
        cur = self.base
        for k in sorted(self.lr):
            if k <= s:
                cur = self.lr[k]
        return cur

    def lr_gen_of(self, t):
        return self.rates(t - self.T0)[0]

    def lr_reg_of(self, t):
        return self.rates(t - self.T0)[1]

    def lr_max(self):
        return max(max(v) for v in list(self.lr.values()) + [self.base])

    def probes_at(self, s):
        """Rows whose item is in the training batch of relative step s (with value 0)."""
        return [i for i in range(self.P) if s in self.train[i]]

    def sync_points(self, i):
        """Relative steps through which some catch-up brings row i (besides the final flush at S)."""
        pts = set(self.reloads)
        for s in self.train[i]:
            pts.update((s - 1, s))
        pts.update(s for s, rows in self.pred_after.items() if i in rows)
        if self.dense_at:
            pts.update((self.dense_at - 1, self.dense_at))
        return sorted(x for x in pts if 0 < x <= self.S)

    def _phases(self, i):
        """Row i's (lo, hi, state at lo or None = carried over) ranges of relative steps."""
        r0 = self.groups[i][0]
        st = {k: self.states[k][i].copy() for k in KEYS}
        if not r0:
            return [(0, self.S, st)]
        zero = {k: (st[k].copy() if k == "p" else np.zeros_like(st[k])) for k in KEYS}
        return [(0, r0, zero), (r0, self.S, st)]

    def _through(self, i, fn, upto, **kw):
        """Row i from T0 through relative step `upto`: (float64 state, summed tails, bounds with p's carried over,
        fn's own state) - fn = replay64 (reference only) or replay32 (also the fp32 restatement)."""
        pts = self.sync_points(i)
        st64 = st32 = None
        tails, tol_p, tol = 0.0, 0.0, None
        for lo, hi, start in self._phases(i):
            if lo >= upto:
                break
            hi = min(hi, upto)
            if st64 is None:
                st64, st32 = start, start
            else:                                   # a reload: the moments are rewritten, p stays
                st64 = dict(start, p=st64["p"])
                st32 = dict(start, p=st32["p"])
            args = (self.T0 + lo, [self.T0 + x for x in pts if lo < x < hi], self.T0 + hi, self.lr_gen_of, self.lr_reg_of)
            new64, tail, tol = _walk(st64, *args)
            if fn is replay32:
                st32 = replay32(st32, *args, **kw)
            st64 = new64
            tails = tails + tail
            tol = dict(tol, p=tol["p"] + tol_p)       # (a reload rewrites the moments exactly: only p's budget carries over)
            tol_p = tol["p"]
        return st64, tails, tol, st32

    def reference(self, i):
        """Row i at the end of the run: (replay64's state, dropped tail, bounds)."""
        return self._through(i, replay64, self.S)[:3]

    def restated(self, i, **kw):
        """... and replay32's state: (replay64's, bounds, replay32's)."""
        st64, _, tol, st32 = self._through(i, replay32, self.S, **kw)
        return st64, tol, st32

    def increment64(self, i, s, rates):
        """p's increment (both optimisers) of row i at relative step s under `rates`, from the float64 state before it."""
        if s > 1:
            st = self._through(i, replay64, s - 1)[0]
            for lo, _, start in self._phases(i):
                if lo == s - 1 and lo:              # reloaded right in front of step s
                    st = dict(start, p=st["p"])
        else:
            st = self._phases(i)[0][2]
        st = {k: np.asarray(st[k], dtype=np.float64) for k in KEYS}
        sg, sr, ib = step_scalars(self.T0 + s, rates[0], rates[1])
        m1, v1 = st["m1"] - B1C * st["m1"], B2 * st["v1"]
        m3, v3 = st["m3"] - B1C * st["m3"], B2 * st["v3"]
        return -sg * m1 / (np.sqrt(v1) * ib + EPS) - sr * m3 / (np.sqrt(v3) * ib + EPS)
