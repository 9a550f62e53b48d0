"""Case tables, references and bounds for the scans and reductions between a flight and what is read off it, at production grid sizes and
ragged edges: the GAE scan with its one-pass statistics (gae_kernel, gae_finalize_kernel), the advantage sums and the normalisation
(sum_partial_kernel, sum_finalize_kernel, adv_apply_kernel) and the streaming score card (score_kernel, score_read_kernel,
score_summary_*_kernel).  Not collected: tests/test_scan_edges_cpu.py asserts of these host statements everything
tests/test_gpu_scan_edges.py relies on, and the GPU file compares the kernels with them.

LAUNCH ARITHMETIC, restated from the launchers (dpenv_kernels.hip): gae_form / gae_partials (two columns per lane when n is even, the float
blocks 8-byte and `end` 2-byte aligned, else one; a workgroup per 64 lanes), reduce_grid / sum_geometry (a workgroup of 256 per 1 024
floats, capped at 2 048, float4 reads when the base is 16-byte aligned, else the scalar loop), score_partials (a wave per 64 envs).

BOUNDS, u = 2^-24, all derived, none from a kernel's output.
  GAE against float64 (gae_f64_bound): every f32 operation of delta = (r + gamma * vnext) - v, acc = delta + (gamma * lam) * acc and
    g = r + gamma * g adds u x the sum of the magnitudes entering it (a product: its magnitude; gamma * lam itself is one rounding, carried
    by |acc|); the carried error is multiplied by |gamma * lam| (adv) or |gamma| (ret); error and carry reset at a path end.  Magnitudes
    are those of the float64 scan plus the error carried so far, and the rounding terms are widened by (1 + 2^-20) for what is second
    order in u (at most four roundings meet in one step: (1 + u)^4 - 1 - 4 u < 2^-20 x 4 u).
  Double sums (sum_bound): |got - fsum(terms)| <= K 2^-53 fsum |terms|, K the double additions along the longest chain: the lane's own
    terms, 6 wave steps, ceil(partials / 256) fold steps, 8 tree steps (k_gae_stats, k_score_summary); sum_partial_kernel adds its 4-wave
    fold (k_sum).  The terms are the f32 per-element values restated in NumPy float32 ((x - m) and d * d are single roundings: the build
    uses -ffp-contract=off); a square of an f32 formed in double is exact.
  Normalisation (norm_reference): y = (x - m) * inv in float64 with m and inv formed as include/dpenv.h states - one-pass: mu = s1 / N,
    var = max(s2 / N - mu^2, 0) in double, the denominator f32(f32(sqrt(var)) + 1e-8f); three-pass: from the f32 scalars.  Bound 3 u |y|
    (subtraction, reciprocal, product) + u |m| |inv| for the one-pass form's cast of the mean.  Statistics that carry K double additions
    move var by at most (2 K + 5) 2^-53 s2 / N (2 K from the two sums, 5 from the roundings of the formula itself, every one of which is
    relative to a quantity <= s2 / N) and mu by K 2^-53 fsum |x| / N; both reach y through inv - the f32 roundings of the denominator are
    monotone, so the restated chain evaluated at var -+ delta_var encloses the kernel's - and through the subtraction.
  Score card: no bound.  score_update is the per-row update of include/dpenv.h written once in NumPy (float32 per-sample terms in the
    stated order, float64 sums in row order) and read() is held to it bit for bit; the summary's min and max are read()'s exactly and
    its sums fall under sum_bound."""
import functools
import math

import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
U53 = 2.0 ** -53
SECOND_ORDER = 1.0 + 2.0 ** -20
GAE_U, SCORE_U, SUMB, SUM_MAXGRID, FOLD = 8, 2, 256, 2048, 256
END_BYTES = (1, 2, 3, 5, 0x80, 0xFF)
GAMMA_LAM = ((0.99, 0.97), (1.0, 1.0), (0.0, 0.5), (0.5, 0.0))
EPS = F32(1e-8)


def ceil_div(a, b):
    return -(-int(a) // int(b))


# ---- launch arithmetic ----------------------------------------------------------------------------------------------------------------
def gae_form(n, float_offset=0, end_offset=0):
    """Columns per lane launch_gae chooses for blocks whose bases sit float_offset / end_offset bytes behind a 16-byte boundary."""
    return 2 if (n % 2 == 0 and float_offset % 8 == 0 and end_offset % 2 == 0) else 1


def gae_partials(n, V):
    return ceil_div(ceil_div(n, V), 64)


def gae_workspace_bytes(n):
    return ceil_div(n, 64) * 2 * 8


def reduce_grid(count):
    return max(1, min(SUM_MAXGRID, ceil_div(count // 4, SUMB)))


def sum_geometry(count, offset=0):
    """grid, float4 count and the trips of the two grid-stride loops of sum_partial_kernel / adv_apply_kernel."""
    grid = reduce_grid(count)
    nvec = count // 4 if offset % 16 == 0 else 0
    stride = grid * SUMB
    return dict(grid=grid, nvec=nvec, stride=stride, vec_trips=ceil_div(nvec, stride), tail_trips=ceil_div(count - 4 * nvec, stride))


def score_partials(n):
    return ceil_div(n, 64)


def k_fold(parts):
    return ceil_div(parts, FOLD) + 8


def k_gae_stats(T, n, V):
    return V * T + 6 + k_fold(gae_partials(n, V))


def k_score_summary(n):
    return 1 + 6 + k_fold(score_partials(n))


def k_sum(count, offset=0):
    g = sum_geometry(count, offset)
    return 4 * g['vec_trips'] + g['tail_trips'] + 6 + SUMB // 64 + k_fold(g['grid'])


def fsum_terms(terms):
    """(fsum, fsum of magnitudes) of the terms as doubles."""
    a = np.asarray(terms, F64).ravel()
    tot = math.fsum(a.tolist())
    if a.size and (a.min() >= 0.0):
        return tot, tot
    return tot, math.fsum(np.abs(a).tolist())


def sum_bound(K, abs_total):
    return K * U53 * abs_total


# ---- GAE --------------------------------------------------------------------------------------------------------------------------------
# (T, n): every T of {1, 2, 7, 8, 9, 15, 16, 17, 24, 25, 33} twice (below, on and above one bank of 8 rows, two banks, three, four and one
# row), every n of {1, 2, 3, 63, 64, 65, 126, 128, 130} at least twice (63, 64, 65 live lanes in the scalar and in the two-column form)
GAE_CASES = ((1, 1), (1, 64), (2, 2), (2, 130), (7, 3), (7, 128), (8, 63), (8, 126), (9, 65), (9, 2), (15, 64), (15, 3), (16, 126),
             (16, 65), (17, 128), (17, 1), (24, 130), (24, 63), (25, 64), (25, 126), (33, 65), (33, 128))
GAE_MODES = ('boot', 'last_val', 'neither', 'no_end')
GAE_FORM_CASES = ((17, 130), (9, 64))                    # even n: the two-column form unless a base is carved off its alignment
GAE_PARTIAL_CASES = ((2, 32770), (2, 16385), (1, 65536), (1, 65664))
GAE_PARTIAL_COUNTS = (257, 257, 512, 513)
GAE_PARTIAL_FORMS = (2, 1, 2, 2)


def gae_case_id(c):
    return 'T%d-n%d' % c


def gamma_lam(k):
    return GAMMA_LAM[k % 4]


@functools.lru_cache(maxsize=None)
def gae_inputs(T, n, seed=0):
    """rew, val, boot [T, n] and last_val [n] float32, end [T, n] uint8 with bytes of END_BYTES on a tenth of the samples and, where the
    columns exist: column 0 ends at t = 0 only, 1 at t = T-1 only, 2 on every row, 3 never; one adjacent (even, odd) column pair - columns
    4, 5, or the last such pair of a narrow block - holds (0x80, 0) on one row and (0, 0xFF) on another and nothing else."""
    rng = np.random.RandomState(7000 + 131 * T + n + 7919 * seed)
    rew = rng.randn(T, n).astype(F32)
    val = rng.randn(T, n).astype(F32)
    boot = (rng.randn(T, n) * (rng.rand(T, n) < 0.5)).astype(F32)
    last_val = rng.randn(n).astype(F32)
    end = np.where(rng.rand(T, n) < 0.1, rng.choice(END_BYTES, size=(T, n)), 0).astype(np.uint8)
    if n > 0:
        end[:, 0] = 0; end[0, 0] = 2
    if n > 1:
        end[:, 1] = 0; end[T - 1, 1] = 3
    if n > 2:
        end[:, 2] = 5
    if n > 3:
        end[:, 3] = 0
    if n >= 2:
        c = 4 if n >= 6 else (n - 2) // 2 * 2
        end[:, c:c + 2] = 0
        end[T // 2, c] = 0x80
        if T >= 2:
            end[(T // 2 + 1) % T, c + 1] = 0xFF
    for a in (rew, val, boot, last_val, end):
        a.setflags(write=False)
    return dict(rew=rew, val=val, boot=boot, last_val=last_val, end=end)


def gae_mode_args(inp, mode):
    """(end, boot, last_val) of a mode."""
    return dict(boot=(inp['end'], inp['boot'], None), last_val=(inp['end'], None, inp['last_val']), neither=(inp['end'], None, None),
                no_end=(None, None, inp['last_val']))[mode]


def gae_scan(dtype, rew, val, end, boot, last_val, gamma, lam, end_rule='nonzero', swap_pairs=False, rows=0):
    """The scan of dpenv_gae in NumPy arithmetic of `dtype`, every operation one rounding; float64 takes the float32-rounded gamma and lam.
    The mutants of the CPU test: end_rule='eq1' (`== 1` in place of `!= 0`), swap_pairs (the two columns of a lane take each other's end
    byte), rows=+1 / -1 (the last, partial bank consumes the clamped re-read of row 0 once more / stops one row early)."""
    T, n = rew.shape
    r, v = rew.astype(dtype), val.astype(dtype)
    gm, lm = dtype(F32(gamma)), dtype(F32(lam))
    gl = dtype(gm * lm)
    if end is None:
        e = np.zeros((T, n), bool)
    else:
        e = (end == 1) if end_rule == 'eq1' else (end != 0)
        if swap_pairs and n % 2 == 0:
            e = e.reshape(T, n // 2, 2)[:, :, ::-1].reshape(T, n)
    zero = np.zeros(n, dtype)
    adv, ret = np.zeros((T, n), dtype), np.zeros((T, n), dtype)
    acc, g, vnext = zero, zero, zero
    ts = list(range(T - 1, -1, -1))
    if rows > 0:
        ts.append(0)
    elif rows < 0:
        ts = ts[:-1]
    for t in ts:
        is_end = e[t] | (t == T - 1)
        lv = boot[t].astype(dtype) if boot is not None else (last_val.astype(dtype) if (t == T - 1 and last_val is not None) else zero)
        acc = np.where(is_end, zero, acc)
        g = np.where(is_end, lv, g)
        vnext = np.where(is_end, lv, vnext)
        delta = (r[t] + gm * vnext) - v[t]
        acc = delta + gl * acc
        g = r[t] + gm * g
        vnext = v[t]
        adv[t], ret[t] = acc, g
    return adv, ret


def gae_f64_bound(rew, val, end, boot, last_val, gamma, lam):
    """(adv, ret, bound of adv, bound of ret): the float64 scan with the float32-rounded gamma and lam, and the running bound of the module
    docstring on what a float32 scan of the same rows may differ from it by."""
    T, n = rew.shape
    r, v = rew.astype(F64), val.astype(F64)
    gm, lm = F64(F32(gamma)), F64(F32(lam))
    gl = gm * lm
    agm, agl = abs(gm), abs(gl)
    e = np.zeros((T, n), bool) if end is None else (end != 0)
    zero = np.zeros(n, F64)
    adv, ret, badv, bret = (np.zeros((T, n), F64) for _ in range(4))
    acc, g, vnext, ea, eg = zero, zero, zero, zero, zero
    for t in range(T - 1, -1, -1):
        is_end = e[t] | (t == T - 1)
        lv = boot[t].astype(F64) if boot is not None else (last_val.astype(F64) if (t == T - 1 and last_val is not None) else zero)
        acc, ea, eg = np.where(is_end, zero, acc), np.where(is_end, zero, ea), np.where(is_end, zero, eg)
        g, vnext = np.where(is_end, lv, g), np.where(is_end, lv, vnext)
        gv = gm * vnext                                   # vnext is an input (or a bootstrap): exact
        s = r[t] + gv
        delta = s - v[t]
        e_delta = U * SECOND_ORDER * (np.abs(gv) + (np.abs(r[t]) + np.abs(gv)) + (np.abs(s) + np.abs(v[t])))
        A = np.abs(acc) + ea                              # what the f32 scan may carry
        ea = e_delta + agl * ea + U * SECOND_ORDER * (2.0 * agl * A + (np.abs(delta) + e_delta + agl * A))
        acc = delta + gl * acc
        G = np.abs(g) + eg
        eg = agm * eg + U * SECOND_ORDER * (agm * G + (np.abs(r[t]) + agm * G))
        g = r[t] + gm * g
        vnext = v[t]
        adv[t], ret[t], badv[t], bret[t] = acc, g, ea, eg
    return adv, ret, badv, bret


_ORACLES = {}


def oracle(dtype):
    if dtype not in _ORACLES:
        from oracle import oracle as O
        _ORACLES[dtype] = O.Oracle(O.make_config(), dtype)
    return _ORACLES[dtype]


def oracle_gae(dtype, end, boot, last_val, rew, val, gamma, lam):
    """The project's standard: the oracle's scan in float32, or in float64 with the float32-rounded gamma and lam."""
    return oracle(dtype).gae(rew, val, end=end, boot=boot, last_val=last_val, gamma=float(F32(gamma)), lam=float(F32(lam)))


@functools.lru_cache(maxsize=None)
def gae_reference(T, n, mode, gamma, lam, seed=0):
    """dict(adv32, ret32: the oracle's float32 scan; adv64, ret64: its float64 scan; badv, bret: the bound between the two)."""
    inp = gae_inputs(T, n, seed)
    end, boot, lv = gae_mode_args(inp, mode)
    a32, r32 = oracle_gae(F32, end, boot, lv, inp['rew'], inp['val'], gamma, lam)
    a64, r64 = oracle_gae(F64, end, boot, lv, inp['rew'], inp['val'], gamma, lam)
    _, _, badv, bret = gae_f64_bound(inp['rew'], inp['val'], end, boot, lv, gamma, lam)
    return dict(adv32=a32, ret32=r32, adv64=a64, ret64=r64, badv=badv, bret=bret)


def gae_stats_reference(adv32):
    """((fsum adv, fsum |adv|), (fsum adv^2, the same)) of float32 advantages; the squares are formed in double, where they are exact."""
    a = adv32.astype(F64)
    return fsum_terms(a), fsum_terms(a * a)


def gae_block_partials(adv32, V):
    """Per-workgroup (sum, sum of squares) of the advantages, a workgroup = 64 lanes of V columns: the partials gae_finalize_kernel folds."""
    T, n = adv32.shape
    a = adv32.astype(F64)
    w = 64 * V
    return [(math.fsum(a[:, b * w:(b + 1) * w].ravel().tolist()), math.fsum((a[:, b * w:(b + 1) * w] ** 2).ravel().tolist()))
            for b in range(gae_partials(n, V))]


def fold_model(partials, limit=None):
    """The finalize kernels' fold as a sum: thread k takes partials k, k + 256, ...; `limit` = 256 is the mutant that stops after each
    thread's first partial."""
    p = list(partials)
    return math.fsum(p if limit is None else p[:limit])


# ---- sums and apply -------------------------------------------------------------------------------------------------------------------
SUM_COUNTS = (1, 3, 4, 5, 1023, 1025, 262149, 2097152, 2097153, 4194311)
SUM_OFFSETS = (0, 4)                                     # bytes behind a 16-byte boundary: float4 reads / the scalar fallback
SUM_BLOCKS = ('const', 'offset')


@functools.lru_cache(maxsize=None)
def sum_block(kind, count):
    if kind == 'const':
        x = np.full(count, 1.5, F32)
    else:
        x = (1000.0 + 0.01 * np.random.RandomState(900 + count % 997).randn(count)).astype(F32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def sum_reference(kind, count):
    """dict(s1, s1abs: fsum of x and of |x|; mean: f32(s1 / count), the scalar dpenv_adv_sumsq and dpenv_adv_apply are given;
    ssq: fsum of f32((x - mean)^2) with f32 (x - mean); std: f32(sqrt(f32(ssq) / count)); s2: fsum of x^2 formed in double)."""
    x = sum_block(kind, count)
    s1, s1abs = fsum_terms(x)
    mean = F32(s1 / count)
    d = x - mean
    ssq, _ = fsum_terms(d * d)
    std = F32(np.sqrt(F32(ssq) / F32(count)))
    s2, _ = fsum_terms(x.astype(F64) ** 2)
    return dict(s1=s1, s1abs=s1abs, mean=mean, ssq=ssq, std=std, s2=s2)


def sum_model(x, offset=0, one_trip=False):
    """fsum of the elements sum_partial_kernel's two grid-stride loops visit; one_trip is the mutant whose loops make a single trip."""
    count = x.size
    g = sum_geometry(count, offset)
    if not one_trip:
        return math.fsum(x.astype(F64).tolist())
    nv = min(g['nvec'], g['stride'])
    head = x[:4 * nv]
    tail = x[4 * g['nvec']:min(count, 4 * g['nvec'] + g['stride'])]
    return math.fsum(head.astype(F64).tolist()) + math.fsum(tail.astype(F64).tolist())


def inv_chain(var, eps=EPS):
    """1 / f32(f32(sqrt(var)) + eps) in float64: the one-pass form's denominator as the kernel's f32 roundings form it."""
    return 1.0 / F64(F32(F32(np.sqrt(max(float(var), 0.0))) + F32(eps)))


def norm_reference(x, mean=None, std=None, stats=None, total=None, K=0, s1abs=0.0, eps=EPS):
    """(y float64, bound) of adv <- (adv - mean) / (std + 1e-8) for float32 x.  Three-pass: mean, std are the f32 scalars.  One-pass:
    stats = (s1, s2) doubles over `total` samples that carry K double additions each (K = 0: correctly rounded sums), s1abs = fsum |x|
    over them.  eps is a parameter for the mutant of the CPU test."""
    x64 = x.astype(F64)
    if stats is None:
        m, inv = F64(mean), 1.0 / F64(F32(F32(std) + F32(eps)))
        y = (x64 - m) * inv
        return y, 3.0 * U * SECOND_ORDER * np.abs(y)
    s1, s2, N = F64(stats[0]), F64(stats[1]), F64(total)
    mu = s1 / N
    ex2 = s2 / N
    var = max(ex2 - mu * mu, 0.0)
    inv = inv_chain(var, eps)
    dvar = (2 * max(K, 1) + 5) * U53 * ex2
    dmu = max(K, 1) * U53 * (s1abs / N)
    dinv = max(abs(inv_chain(var - dvar, eps) - inv), abs(inv_chain(var + dvar, eps) - inv))
    y = (x64 - mu) * inv
    bound = 3.0 * U * SECOND_ORDER * np.abs(y) + U * abs(mu) * inv + np.abs(x64 - mu) * dinv + dmu * (inv + dinv)
    return y, bound


# ---- score card -----------------------------------------------------------------------------------------------------------------------
R2D = F32(57.295779513082323)
SCORE_SLOTS = ('iae', 'work0', 'work1', 'work2', 'ret', 'len', 'episodes', 'ep_iae', 'ep_work0', 'ep_work1', 'ep_work2', 'ep_ret', 'ep_len')
SCORE_T = (1, 2, 3, 4, 5)
SCORE_N = (1, 63, 64, 65)
OBS_STRIDES = (3, 6, 9, 12)
ACT_STRIDES = (3, 7, 8)
DONE_PATTERNS = ('every', 'none', 'first_last')
SCORE_SUMMARY_N = (16385, 32832)
SCORE_SUMMARY_PARTIALS = (257, 513)


def score_cases():
    """(T, n, obs_stride, bf16, act_stride): the 20 (T, n), the strides and the obs type dealt so that each stride meets both types and
    every T and n."""
    out = []
    for k, (T, n) in enumerate((T, n) for T in SCORE_T for n in SCORE_N):
        ti, ni = k // 4, k % 4
        out.append((T, n, OBS_STRIDES[(ni + ti) % 4], bool((ti + ni // 2) % 2), ACT_STRIDES[(k + k // 3) % 3]))
    return tuple(out)


SCORE_CASES = score_cases()


def score_case_id(c):
    return 'T%d-n%d-obs%d%s-act%d' % (c[0], c[1], c[2], 'bf16' if c[3] else 'f32', c[4])


def score_consts():
    """The defaults of dpenv_score_default_io as include/dpenv.h states them, float32."""
    from ml4ca_amd import evaluate as EV
    coeff = [F32(EV.KQ0[w] * 2 * math.pi * EV.RHO * EV.DIAMETER[w] ** 5) for w in ('bow', 'stern', 'stern')]
    return dict(dt=F32(0.2), norm=np.array([5.0, 5.0, 25.0], F32), coeff=np.array(coeff, F32), rps=np.array([33.0, 11.0, 11.0], F32))


def bf16_round(x):
    """float32 -> the nearest bfloat16 (ties to even) as float32: what torch's .to(bfloat16) stores and the kernel widens."""
    b = np.ascontiguousarray(x, F32).view(np.uint32).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return b.astype(np.uint32).view(F32).reshape(np.shape(x))


@functools.lru_cache(maxsize=None)
def score_rows(T, n, obs_stride, act_stride, bf16=False, seed=0, negative_rew=False):
    """Seeded rows: pose errors of order 2 m / 0.3 rad (bf16-representable when bf16), integ, actions in +-1.3 with both signs and exact
    zeros (the clip and sgn(0) are met), rewards in [-1, 3.5] or, negative_rew, in [-3.5, -0.5]."""
    rng = np.random.RandomState(4000 + 17 * T + n + 1009 * seed)
    obs = rng.normal(0.0, 1.0, size=(T, n, obs_stride)).astype(F32)
    obs[..., 0:2] *= F32(2.0)
    obs[..., 2] *= F32(0.3)
    if bf16:
        obs = bf16_round(obs)
    integ = (rng.uniform(-1, 1, size=(T, n, 3)) * np.array([0.02, 0.03, 0.004])).astype(F32)
    act = rng.uniform(-1.3, 1.3, size=(T, n, act_stride)).astype(F32)
    act[rng.uniform(size=act.shape) < 0.05] = 0.0
    rew = rng.uniform(-3.5, -0.5, size=(T, n)).astype(F32) if negative_rew else rng.uniform(-1.0, 3.5, size=(T, n)).astype(F32)
    for a in (obs, integ, act, rew):
        a.setflags(write=False)
    return dict(obs=obs, integ=integ, act=act, rew=rew)


def done_pattern(kind, T, n):
    """every: a non-zero byte of END_BYTES on every row; none; first_last: env i ends at t = 0 (i % 3 == 0), at t = T-1 (i % 3 == 1) or
    at both (i % 3 == 2)."""
    d = np.zeros((T, n), np.uint8)
    i = np.arange(n)
    if kind == 'every':
        d[:] = np.array(END_BYTES, np.uint8)[(np.arange(T)[:, None] + i[None, :]) % len(END_BYTES)]
    elif kind == 'first_last':
        d[0, i % 3 != 1] = 0x80
        d[T - 1, i % 3 != 0] = 2
    return d


def score_fresh(n):
    z = lambda *s: np.zeros(s, F64)
    return dict(iae=z(n), w=z(n, 3), ret=z(n), c_iae=z(n), c_w=z(n, 3), c_ret=z(n), qp=np.zeros(n, F32), pp=np.zeros((n, 3), F32),
                len=np.zeros(n, np.int64), has_prev=np.zeros(n, bool), episodes=np.zeros(n, np.int64), c_len=np.zeros(n, np.int64))


def score_update(st, blk, consts, cut_at_end=False, rows=0):
    """The per-row update of include/dpenv.h ("Per-row update") for one block, in place on st: float32 per-sample terms in the stated
    order, float64 sums in row order.  blk: obs [T, n, >= 3] float32 (bf16 already widened), act [T, n, >= 3], rew [T, n], done [T, n]
    uint8, integ [T, n, 3]; any may be missing.  rows=+1 / -1 are the mutants of the CPU test: the last, partial bank consumes the clamped
    re-read of row T-1 once more / stops one row early."""
    obs, act, rew, done, integ = (blk.get(k) for k in ('obs', 'act', 'rew', 'done', 'integ'))
    T = next(a.shape[0] for a in (obs, act, rew) if a is not None)
    n = st['iae'].shape[0]
    dt, norm, coeff, rps = consts['dt'], consts['norm'], consts['coeff'], consts['rps']
    half, hundred = F32(0.5), F32(100.0)
    ts = list(range(T)) + ([T - 1] if rows > 0 else [])
    for t in (ts[:-1] if rows < 0 else ts):
        q, P = np.zeros(n, F32), np.zeros((n, 3), F32)
        if obs is not None:
            e = obs[t, :, :3].astype(F32)
            if integ is not None:
                e = e - integ[t]
            e0 = e[:, 0] / norm[0]
            e1 = e[:, 1] / norm[1]
            e2 = (e[:, 2] * R2D) / norm[2]
            q = np.sqrt((e0 * e0 + e1 * e1) + e2 * e2)
        if act is not None:
            nn = np.minimum(np.maximum(act[t, :, :3] * hundred, -hundred), hundred)
            x = (nn / hundred) * rps[None, :]
            P = (np.sign(nn) * coeff[None, :]) * ((x * x) * x)
        hp = st['has_prev']
        if obs is not None:
            st['iae'] = st['iae'] + np.where(hp, ((half * (q + st['qp'])) * dt).astype(F64), 0.0)
        if act is not None:
            st['w'] = st['w'] + np.where(hp[:, None], ((half * (P + st['pp'])) * dt).astype(F64), 0.0)
        if rew is not None:
            st['ret'] = st['ret'] + rew[t].astype(F64)
        st['len'] = st['len'] + 1
        st['qp'], st['pp'], st['has_prev'] = q.astype(F32), P.astype(F32), np.ones(n, bool)
        close = ((done[t] != 0) if done is not None else np.zeros(n, bool)) | (bool(cut_at_end) and t == T - 1)
        st['c_iae'] = st['c_iae'] + np.where(close, st['iae'], 0.0)
        st['c_w'] = st['c_w'] + np.where(close[:, None], st['w'], 0.0)
        st['c_ret'] = st['c_ret'] + np.where(close, st['ret'], 0.0)
        st['c_len'] = st['c_len'] + np.where(close, st['len'], 0)
        st['episodes'] = st['episodes'] + close
        st['iae'], st['ret'] = np.where(close, 0.0, st['iae']), np.where(close, 0.0, st['ret'])
        st['w'] = np.where(close[:, None], 0.0, st['w'])
        st['len'] = np.where(close, 0, st['len'])
        st['has_prev'] = st['has_prev'] & ~close
        st['qp'] = np.where(close, F32(0.0), st['qp'])
        st['pp'] = np.where(close[:, None], F32(0.0), st['pp'])
    return st


def score_read(st):
    """float64 [13, n]: the read slots in the order of DPENV_SCORE_*."""
    return np.stack([st['iae'], st['w'][:, 0], st['w'][:, 1], st['w'][:, 2], st['ret'], st['len'].astype(F64), st['episodes'].astype(F64),
                     st['c_iae'], st['c_w'][:, 0], st['c_w'][:, 1], st['c_w'][:, 2], st['c_ret'], st['c_len'].astype(F64)])


def score_pieces(T, piece):
    """Row ranges of a block of T rows cut into pieces of `piece` rows (0: the whole block)."""
    return [(0, T)] if not piece else [(t, min(t + piece, T)) for t in range(0, T, piece)]


def slice_block(blk, t0, t1):
    return {k: (v if v is None else v[t0:t1]) for k, v in blk.items()}


@functools.lru_cache(maxsize=None)
def summary_rows(n):
    """T = 2 rows for the summary: every env its own values, all returns negative; the open iae falls with the env index (its minimum sits
    on env n-1) and the open return rises with it (its maximum, the return closest to 0, sits on env n-1)."""
    i = np.arange(n, dtype=F64)
    obs = np.zeros((2, n, 3), F32)
    obs[:, :, 0] = (1.0 + (n - 1 - i) / n).astype(F32)[None, :]
    obs[1, :, 1] = 0.5
    act = np.zeros((2, n, 3), F32)
    act[:, :, 0] = (0.1 + 0.8 * i / n).astype(F32)[None, :]
    act[:, :, 1] = (-0.2 - 0.5 * i / n).astype(F32)[None, :]
    act[:, :, 2] = (0.9 - 0.8 * i / n).astype(F32)[None, :]
    rew = np.empty((2, n), F32)
    rew[0] = (-3.0 + 2.0 * i / n).astype(F32)
    rew[1] = -0.25
    for a in (obs, act, rew):
        a.setflags(write=False)
    return dict(obs=obs, act=act, rew=rew)


def summary_model(vals, neutral_zero=False, limit=None):
    """(sum, min, max) of one read slot as the two summary stages form them over waves of 64 envs; neutral_zero is the mutant whose dead
    lanes and fold registers start from 0 in place of +-inf, limit = 256 the one whose fold stops after each thread's first partial."""
    v = np.asarray(vals, F64)
    parts = [v[b * 64:(b + 1) * 64] for b in range(score_partials(v.size))]
    if limit is not None:
        parts = parts[:limit]
    kept = np.concatenate(parts)
    lo, hi = float(kept.min()), float(kept.max())
    if neutral_zero:
        lo, hi = min(lo, 0.0), max(hi, 0.0)
    return math.fsum(kept.tolist()), lo, hi
