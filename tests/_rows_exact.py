"""Rows on which LayerNorm's statistics are exact, an fp64 reference, a per-element bound, and a CPU emulation of the row kernels.

The row kernels (actionmesh_amd/csrc/am_norm.hip, layernorm_f32_kernel of am_f32.hip) sum a row, subtract the mean, sum the squared
deviations, take a reciprocal square root and scale.  A row here is  x_c = m + s d_c  with s a power of two, m a multiple of s and
d_c integers in {+-1, +-3}: a quarter of the columns at +-3, as many +3 as -3 and as many +1 as -1 (C % 8 == 4, fp32 rows only:
one more 3 on one side, three more 1 on the other), so that  sum d = 0  and  sum d^2 = 3 C.  The positions are a seeded permutation
of the WHOLE row - group sums over 8 / 64 / 256 neighbouring columns are not zero (asserted), so the order of a reduction is visible
to every intermediate value and to none of the results: with  sum |x| / s < 2^24  and  sum d^2 < 2^24  (asserted) every fp32 partial
sum of the row and of the squared deviations is exact in any order.  The mean is m, x - mean is s d and the sum of squares 3 C s^2,
none of them rounded.  What is left of a correct kernel's error is counted from its source (`K1`, `K2` below), not fitted.

Row profiles; `cycle` rows take them in turn with the row index, so the four rows of a workgroup differ (eps = 1e-5):
  plain         m = 0, s = 1
  offset        m = +-OFFSET s, the sign alternating: the largest m < 2^11 with m +- 1 and m +- 3 exact in the storage type: 509 in
                bf16, 2047 in f16 (odd, so that the four values are even, where the type's spacing is 2) and in fp32 - 4096
                columns still sum below 2^24.  |mean| / sigma is 294 / 1182 / 1182.  A variance formed as E[x^2] - mean^2 loses
                its digits on the f16 and fp32 rows (x^2 has 22 bits and every sum of 32 or more of them drops the low ones; an
                m of 2^11 would hide that: the squares' low bits are then d^2 alone and their roundings cancel).  bf16's 8 bits
                do not reach such rows: 4096 squares of 18 bits lose nothing that a 16-bit output shows
  eps_dominant  s = 2^-10: var = 3 2^-20 = 2.9e-6 < eps
  constant      every d = 0 (x = 7): var = 0, the output is b rounded to the output type, exactly
`unit` rows (a call of their own: eps goes through the API): s = 1/2 with eps = 0.25, so var + eps = 1 exactly and rstd should be
1; m = 0 or +-OFFSET / 2.  Whatever these rows measure of rstd is the device's reciprocal square root at 1.0.

Weights: w = +-k / 8, k in 4 .. 15 (|w| in [0.5, 2), mixed signs).  b, multiples of 1/8:  "general" in [-2, 2] (w xhat and b may
cancel: the bound is on the terms, so it holds);  "zero";  "nocancel" |b| in [5, 8]: |w xhat| <= 2 * 3 / sqrt 3 < 3.5 in every
profile, so |w xhat + b| >= |b| - 3.5 >= max(|b|, |w xhat|) / 4 (asserted).

Reference: fp64 from the operands,  ref = w (x - mean) / sqrt(var + eps) + b  with eps the float32 the API passes.
Bound, per element:  0.5 spacing_out(ref) + 2^-24 (K1 |w (x - mean) rstd| + K2 |ref|).  spacing_out is the output type's spacing
AT ref (not u |ref|, up to twice looser; constant below the smallest normal).  Counted on `(v - mean) * rstd * w + b` of
layernorm_kernel / add_layernorm_f32_kernel, in units of 2^-24 relative to the term  t = w (x - mean) rstd:
  sum, mean, x - mean, sq, sq / C    exact on these rows (IEEE division of an exactly divisible quotient)          0
  var + eps                          one rounding, halved by the square root                                         0.5
  rsqrtf                             RSQRT_ULPS fp32 spacings = 2 RSQRT_ULPS units                                   2
  (x - mean) * rstd                  one rounding                                                                    1
  ... * w                            one rounding                                                                    1
  ... + b                            one rounding of the sum (none where the compiler contracts it into an fma)      K2 = 1
  the output                         one rounding to the 16-bit type: the half spacing
K1 = 4.5, K2 = 1.  layernorm_f32_kernel forms 1.0f / sqrtf(var + eps): a correctly rounded root (1 unit) and a correctly rounded
division (1) for the rsqrtf (2) - K1 = 4.5 again - and its `+ b` IS the rounding of the fp32 output: K2 = 0, spacing of fp32.
RSQRT_ULPS = 1: no document shipped with the toolchain states rsqrtf's accuracy, so it is the error measured on the `unit` rows
(tests/test_rows_exact_gpu.py::test_unit_rows_measure_the_device_rsqrt - seen: 0 spacings, rstd == 1.0f on every row, both builds) plus one ulp of
margin; HIP's published table of device functions gives 1 ulp for rsqrtf as well.
K1 is multiplied by (1 + 2^-20) for the products of the terms above.

Statistics (row_stats, layernorm(stats_out=), row_stats_finalize): per row against fp64.  C % 256 != 0 is the two-pass form: the
mean is m exactly (asserted bit for bit) and rstd carries `var + eps` and the rsqrtf, (0.5 + 2 RSQRT_ULPS) 2^-24.  C % 256 == 0 is
the canonical form of am_common.h: the (mean, M2) of a 256-column slice are exact on these rows (row_part8 and five
row_part_merge_equal levels: every value is a multiple of s / 256 resp. s^2 / 256 well inside 24 bits - asserted on the fp64 parts),
the slices are merged left to right by row_stats_merge with w = 256 / tot rounded, so `stats_bound` walks that chain in fp64 with a
running error of each rounding it contains (d, w, the fma of the mean; d * d, n * w, m2 + qj, the fma of M2; M2 / n, + eps, rsqrtf).
For a row of the `offset` profile the mean's bound is a few 2^-24 (|m| + 3 s), and rstd's a few 2^-24 plus what the mean's error does to
d = mj - mean.

Head split (head_post_kernel, 128 channels per (token, head)): the vector is s d with the same pattern, so the mean square is 3 s^2
and ss = 384 s^2 exact.  Vectors cycle with token + head:  plain s = 1;  tiny s = 2^-11, mean square 7.2e-7 < eps = 1e-6;  zero
(the outputs must be exactly 0).  w_q / w_k = k / 8, k in 4 .. 15.  RoPE tables: multiples of 1/8 in [-1, 1] per (frame, channel
pair), not on the unit circle - the kernel does not care and dyadic values make the reference unambiguous; frames 1, 2, 3 are pinned
to (cos, sin) = (1, 0), (0, 1), (0, -1).  Counted on head_post_kernel and rope_rotate (am_common.h), units of 2^-24:
  ss (fma chain + butterfly), ss * (1 / 128)    exact                                                               0
  + eps                                          one rounding, halved by the root                                    0.5
  rsqrtf                                                                                                             2
  (v * r) * w                                    two roundings                                                       2
      -> without RoPE  0.5 spacing_out(ref) + 4.5 2^-24 |ref|
  b * s, b * c                                   one rounding of the product that enters the fma as its addend       1
  fma(a, c, -bs), fma(a, s, bc)                  one rounding of the result, at most 2^-24 (|x0 c| + |x1 s|)         1
      -> with RoPE     0.5 spacing_out(ref) + 6.5 2^-24 (|x0 c| + |x1 s|): the two products may cancel, the bound is on them
Without w_q / w_k the kernel does not normalise: the products of s d with multiples of 1/8 are exact, and the output must be the
fp64 value rounded once - bit for bit (`head_check` asserts that instead of the bound).

Fold preparation (ln_fold_weight_kernel): W = +-k 2^(e - 6) with k < 16 (4 significant bits), gamma = k / 8 with k in 1 .. 15, beta
and bias multiples of 1/8: W gamma has 8 significant bits - exact in both 16-bit types - and colsum, d are sums of multiples of
2^-9 far below 2^24 of them: wf, colsum and d equal the fp64 values bit for bit.

Unforeseen rounding sites (a form whose bound carries an `extra` term): none."""
import torch

U24 = 2.0 ** -24
EPS = 1e-5
HEAD_EPS = 1e-6
UNIT_EPS = 0.25
RSQRT_ULPS = 1.0
SLACK = 1.0 + 2.0 ** -20
K1 = (0.5 + 2.0 * RSQRT_ULPS + 2.0) * SLACK
K2 = {"bf16": 1.0, "f16": 1.0, "f32": 0.0}
K_HEAD_NORM = (0.5 + 2.0 * RSQRT_ULPS + 2.0) * SLACK
K_HEAD_ROPE = K_HEAD_NORM + 2.0 * SLACK
# storage / output formats: (torch type, significant bits, exponent of the smallest normal)
FORMATS = {"bf16": (torch.bfloat16, 8, -126), "f16": (torch.float16, 11, -14), "f32": (torch.float32, 24, -126)}
NAME = {torch.bfloat16: "bf16", torch.float16: "f16", torch.float32: "f32"}
CYCLE = ("plain", "offset", "eps_dominant", "constant")
B_MODES = ("general", "zero", "nocancel")
LADDER = 512                      # columns per chunk count of launch_layernorm / am_add_layernorm_f32: NCH from ceil(C / 512)
LADDER_F32 = 256                  # of am_layernorm_f32: NCH in {1, 2, 4, 8, 16} from ceil(C / 256)
WIDTHS = [8, 24, 264, 512, 520, 1024, 1032, 2048, 2056, 4088, 4096]
WIDTHS_F32 = [4, 100, 256, 260, 512, 516, 1024, 1028, 2048, 2052, 4096]
ROWS = [5, 131]


def eps32(eps):
    """The float32 the C ABI receives."""
    return float(torch.tensor(eps, dtype=torch.float32))


def rnd(x, fmt):
    """fp64 -> the format (through fp32, as the kernels hold every value in fp32 first; exact operands lose nothing) -> fp64."""
    return x.float().to(FORMATS[fmt][0]).double()


def offset_of(fmt):
    """Largest integer m < 2^11 with m +- 1 and m +- 3 exact in the format."""
    cand = torch.arange(2047, 3, -1, dtype=torch.float64)
    ok = torch.ones_like(cand, dtype=torch.bool)
    for k in (-3.0, -1.0, 1.0, 3.0):
        ok &= rnd(cand + k, fmt) == cand + k
    return float(cand[ok][0])


def pattern(rows, C, seed):
    """d (rows, C) fp64 integers of the module docstring: sum d = 0, sum d^2 = 3 C, a seeded permutation per row."""
    assert C % 4 == 0
    k = C // 4
    a = (k + 1) // 2                                 # +3s; k - a -3s
    p = (3 * k - 3 * (2 * a - k)) // 2               # +1s
    base = torch.cat([torch.full((n,), v) for n, v in ((a, 3.0), (k - a, -3.0), (p, 1.0), (3 * k - p, -1.0))]).double()
    g = torch.Generator().manual_seed(seed)
    d = base[torch.rand((rows, C), generator=g).argsort(-1)]
    if k % 2:                                        # the odd one out changes sides with the row
        d = d * torch.where(torch.arange(rows) % 2 == 0, 1.0, -1.0)[:, None]
    return d


def rows_operands(rows, C, fmt, mode, seed, device="cpu"):
    """x (rows, C) fp64, exact in `fmt`, of mode "cycle" (the four profiles in turn, eps = EPS) or "unit" (eps = UNIT_EPS); checked by
    `rows_conditions`.  -> dict(x, m, s, d, profile (rows,) index into CYCLE or -1, eps)."""
    assert mode in ("cycle", "unit")
    off = offset_of(fmt)
    r = torch.arange(rows)
    d = pattern(rows, C, seed)
    if mode == "cycle":
        prof = r % 4
        sign = torch.where((r // 4) % 2 == 0, 1.0, -1.0).double()
        s = torch.where(prof == 2, 2.0 ** -10, 1.0).double()
        m = torch.where(prof == 1, off * sign, torch.where(prof == 3, 7.0, 0.0)).double()
        d[prof == 3] = 0.0
        eps = EPS
    else:
        prof = torch.full((rows,), -1)
        sign = torch.where((r // 2) % 2 == 0, 1.0, -1.0).double()
        s = torch.full((rows,), 0.5, dtype=torch.float64)
        m = torch.where(r % 2 == 1, 0.5 * off * sign, 0.0).double()
        eps = UNIT_EPS
    op = dict(x=m[:, None] + s[:, None] * d, m=m, s=s, d=d, profile=prof, eps=eps, fmt=fmt)
    rows_conditions(op)
    return {k: v.to(device) if isinstance(v, torch.Tensor) else v for k, v in op.items()}


def rows_conditions(op):
    """What the rows promise, on the operands alone.  Returns the facts it measured."""
    x, m, s, d, fmt = op["x"], op["m"], op["s"], op["d"], op["fmt"]
    rows, C = x.shape
    live = d.abs().amax(-1) > 0
    assert torch.equal(rnd(x, fmt), x), f"a row value is not exact in {fmt}"
    assert bool((torch.log2(s) == torch.log2(s).round()).all()) and bool((m / s == (m / s).round()).all())
    assert bool((d.sum(-1) == 0).all()) and bool((d.pow(2).sum(-1)[live] == 3 * C).all()) and bool((d[~live] == 0).all())
    assert set(d[live].abs().unique().tolist()) <= {1.0, 3.0} and bool(((d[live].abs() == 3).sum(-1) == C // 4).all())
    if C % 8 == 0:
        assert bool(((d[live] == 3).sum(-1) == C // 8).all()) and bool(((d[live] == 1).sum(-1) == 3 * C // 8).all())
    facts = dict(sum_abs=float((x.abs().sum(-1) / s).max()), sum_sq=float(d.pow(2).sum(-1).max()), unbalanced={})
    assert facts["sum_abs"] < 2 ** 24 and facts["sum_sq"] < 2 ** 24, facts
    assert torch.equal(x.mean(-1), m) and torch.equal((x - m[:, None]).pow(2).sum(-1), d.pow(2).sum(-1) * s * s)      # fp64 agrees
    for grp in (8, 64, 256):                         # the permutation is over the whole row, not inside lane / wave / slice groups
        if C >= 2 * grp and bool(live.any()):
            sums = d[live][:, :C // grp * grp].reshape(-1, C // grp, grp).sum(-1)
            threes = (d[live][:, :C // grp * grp].abs() == 3).reshape(-1, C // grp, grp).sum(-1)
            facts["unbalanced"][grp] = float((sums != 0).double().mean())
            assert facts["unbalanced"][grp] > 0.5, f"the pattern is balanced inside groups of {grp} columns"
            assert bool((threes != grp // 4).any()), f"every group of {grp} columns holds its quarter of 3s"
    return facts


def weights(C, b_mode, seed, device="cpu"):
    """(w, b) fp32 on `device`; the values of the module docstring."""
    assert b_mode in B_MODES
    g = torch.Generator().manual_seed(seed)
    k = torch.randint(4, 16, (C,), generator=g).float() / 8
    w = k * (torch.randint(0, 2, (C,), generator=g).float() * 2 - 1)
    if C >= 8:
        assert bool((w > 0).any()) and bool((w < 0).any())
    if b_mode == "general":
        b = torch.randint(-16, 17, (C,), generator=g).float() / 8
    elif b_mode == "zero":
        b = torch.zeros(C)
    else:
        b = torch.randint(40, 65, (C,), generator=g).float() / 8 * (torch.randint(0, 2, (C,), generator=g).float() * 2 - 1)
    return w.to(device), b.to(device)


def ln_reference(x, w, b, eps):
    """fp64 LayerNorm from the operands -> (ref, |w (x - mean) rstd|)."""
    x = x.double()
    mean = x.mean(-1, keepdim=True)
    var = (x - mean).pow(2).mean(-1, keepdim=True)
    t = w.double() * (x - mean) / torch.sqrt(var + eps32(eps))
    ref = t + b.double()
    if float(b.abs().min()) >= 5.0:                  # "nocancel"
        assert bool((ref.abs() >= 0.25 * torch.maximum(t.abs(), b.double().abs().expand_as(t))).all()), "w xhat and b cancel"
    return ref, t.abs()


def spacing(ref, fmt):
    """The format's spacing at |ref| (a power of two takes the spacing above it; the subnormal spacing below the smallest normal)."""
    _, bits, emin = FORMATS[fmt]
    _, e = torch.frexp(ref.double().abs())
    e = torch.where(ref == 0, torch.full_like(e, emin), e - 1).clamp(min=emin)
    return torch.exp2((e - bits + 1).double())


def ln_bound(ref, term, out_fmt, extra=0.0):
    return 0.5 * spacing(ref, out_fmt) + U24 * (K1 * term + K2[out_fmt] * ref.abs()) + extra


def ratio(out, ref, bnd, what):
    """max |out - ref| / bound, printed with its place; a non-finite output counts as infinitely far."""
    err = (out.double() - ref).abs()
    r = torch.where(torch.isfinite(err), err / bnd, torch.full_like(err, float("inf")))
    at = int(r.argmax())
    worst = float(r.flatten()[at])
    place = tuple(int(i) for i in torch.unravel_index(torch.tensor(at), r.shape))
    print(f"exact rows {what}: max err / bound {worst:.3f} at {place}")
    return worst, place


def check(out, ref, bnd, what):
    assert bool(torch.isfinite(out.float()).all()), f"{what}: output not finite"
    worst, place = ratio(out, ref, bnd, what)
    assert worst <= 1.0, f"{what}: |out - ref| = {worst:.3f} x bound at {place}: out {float(out[place])!r}, ref {float(ref[place])!r}"
    return worst


# ---- statistics ------------------------------------------------------------------------------------------------------------------
def slice_parts(x):
    """fp64 (mean, M2) of every 256-column slice -> (rows, nparts, 2), and the slices' counts.  The last may be short (the two-pass
    tail of row_part_kernel): its mean is exact when its count is a power of two, which is asserted - use such widths."""
    C = x.shape[1]
    out, cnt = [], []
    for c0 in range(0, C, 256):
        sl = x[:, c0:c0 + 256].double()
        mu = sl.mean(-1)
        out.append(torch.stack((mu, (sl - mu[:, None]).pow(2).sum(-1)), -1))
        cnt.append(float(sl.shape[1]))
    parts = torch.stack(out, 1)
    assert int(cnt[-1]) & (int(cnt[-1]) - 1) == 0, f"a last slice of {int(cnt[-1])} columns: its mean is rounded"
    assert torch.equal(parts.float().double(), parts), "a slice's (mean, M2) is not exact in fp32"
    return parts, cnt


def stats_reference(x, eps):
    x = x.double()
    mean = x.mean(-1)
    return mean, 1.0 / torch.sqrt((x - mean[:, None]).pow(2).mean(-1) + eps32(eps))


def stats_bound(x, eps, merged):
    """(absolute bound of the mean, relative bound of rstd) per row.  merged False: the two-pass form (mean exact).  True: the slices
    of `slice_parts` merged left to right by row_stats_merge (am_common.h), every rounding of the chain carried as a running error:
      tot = n + nj (exact)   d = mj - mean   w = nj / tot   mean = fma(d, w, mean)   dd = d * d   k = n * w   s = m2 + qj
      m2 = fma(dd, k, s);    then var = m2 / n, var + eps, rsqrtf."""
    u = U24 * SLACK
    rows = x.shape[0]
    z = torch.zeros(rows, dtype=torch.float64, device=x.device)
    e32 = eps32(eps)
    if not merged:
        return z, z + (0.5 + 2.0 * RSQRT_ULPS) * u
    parts, cnt = slice_parts(x)
    n, mean, m2, em, eq = 0.0, z.clone(), z.clone(), z.clone(), z.clone()
    for j, nj in enumerate(cnt):
        mj, qj = parts[:, j, 0], parts[:, j, 1]
        if j == 0:                                   # n = 0: d = mj, w = 1, k = 0 - nothing rounds
            n, mean, m2 = nj, mj.clone(), qj.clone()
            continue
        tot = n + nj
        d, w, k = mj - mean, nj / tot, n * nj / tot
        ed = em + u * (d.abs() + em)                 # d: the mean's error, and one rounding
        new_mean = mean + d * w
        em = em + (ed * w + d.abs() * w * u) * SLACK + u * (new_mean.abs() + em + ed)         # w rounded; the fma's one rounding
        edd = (2 * d.abs() * ed + ed * ed) + u * (d.abs() + ed) ** 2                          # dd: d's error, and one rounding
        es = eq + u * (m2 + qj + eq)                                                          # s = m2 + qj
        new_m2 = m2 + qj + d * d * k
        eq = (edd * k + (d * d + edd) * 2 * u * k) * SLACK + es + u * (new_m2 + edd * k + es)  # k = n * w: two roundings; the fma's
        n, mean, m2 = tot, new_mean, new_m2
    var = m2 / n
    evar = eq / n + u * var + u * (var + e32)        # m2 / n and var + eps, one rounding each
    return em, 0.5 * SLACK * evar / (var + e32) + 2.0 * RSQRT_ULPS * u


def stats_check(st, x, eps, merged, what):
    """st (rows, 2) fp32 (mean, rstd) against fp64 at `stats_bound`; the two-pass mean bit for bit.  Returns (mean ratio, rstd ratio)."""
    assert bool(torch.isfinite(st).all()), f"{what}: statistics not finite"
    mean, rstd = stats_reference(x, eps)
    bm, br = stats_bound(x, eps, merged)
    if merged:
        tiny = torch.finfo(torch.float64).tiny
        rm = ratio(st[:, 0], mean, bm.clamp_min(tiny), f"{what} mean")[0]
    else:
        assert torch.equal(st[:, 0].double(), mean), f"{what}: the two-pass mean of an exactly summable row is its m"
        rm = 0.0
    rr = ratio(st[:, 1], rstd, br * rstd, f"{what} rstd")[0]
    assert rm <= 1.0 and rr <= 1.0, f"{what}: mean {rm:.3f} x bound, rstd {rr:.3f} x bound"
    return rm, rr


def ulps_f32(a, b):
    """|a - b| in fp32 spacings of b (fp32 tensors)."""
    return (a.double() - b.double()).abs() / spacing(b.double(), "f32")


# ---- head split ------------------------------------------------------------------------------------------------------------------
HEAD_PROFILES = ("plain", "tiny", "zero")


def head_operands(rows, heads, nparts, fmt, seed, device="cpu"):
    """x (rows, heads * nparts * 128) fp64: every (token, head, part) vector is s d; the profile cycles with token + head."""
    d = pattern(rows * heads * nparts, 128, seed).view(rows, heads, nparts, 128)
    prof = (torch.arange(rows)[:, None] + torch.arange(heads)[None]) % 3
    s = torch.tensor([1.0, 2.0 ** -11, 0.0], dtype=torch.float64)[prof]
    x = (d * s[:, :, None, None]).reshape(rows, heads * nparts * 128) + 0.0          # + 0.0: the zero vectors are +0, as a linear writes them
    assert torch.equal(rnd(x, fmt), x)
    ms = x.view(rows, heads, nparts, 128).pow(2).mean(-1)
    assert torch.equal(ms, (3 * s * s)[:, :, None].expand_as(ms))
    if rows >= 3:
        assert float(ms[prof == 1].max()) < eps32(HEAD_EPS) < float(ms[prof == 0].min()) and bool((prof == 2).any())
    return x.to(device), prof.to(device)


def head_weights(seed, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    return tuple((torch.randint(4, 16, (128,), generator=g).float() / 8).to(device) for _ in range(2))


def rope_tables(nframes, seed, device="cpu"):
    """(cos, sin) (nframes, 64) fp32, multiples of 1/8 in [-1, 1]; frames 1, 2, 3 pinned to (1, 0), (0, 1), (0, -1)."""
    g = torch.Generator().manual_seed(seed)
    cos, sin = (torch.randint(-8, 9, (nframes, 64), generator=g).float() / 8 for _ in range(2))
    for f, (c, s) in zip((1, 2, 3), ((1.0, 0.0), (0.0, 1.0), (0.0, -1.0))):
        if f < nframes:
            cos[f], sin[f] = c, s
    return cos.contiguous().to(device), sin.contiguous().to(device)


def head_reference(x, heads, nparts, part, w, rope, seq_len, rpf, eps=HEAD_EPS):
    """fp64 statement of one Q / K part -> (ref, terms) as (nseq, heads, seq_len, 128); terms = |x0 c| + |x1 s| (|ref| without RoPE)."""
    rows = x.shape[0]
    xs = x.double().view(rows, heads, nparts, 128)[:, :, part]
    if w is not None:
        xs = xs / torch.sqrt(xs.pow(2).mean(-1, keepdim=True) + eps32(eps)) * w.double()
    terms = xs.abs()
    if rope is not None:
        fr = torch.arange(rows, device=x.device) // rpf
        c, s = (t.double()[fr][:, None, :] for t in rope)                     # (rows, 1, 64)
        x0, x1 = xs.view(rows, heads, 64, 2).unbind(-1)
        xs = torch.stack((x0 * c - x1 * s, x0 * s + x1 * c), -1).flatten(2)
        terms = torch.stack(((x0 * c).abs() + (x1 * s).abs(), (x0 * s).abs() + (x1 * c).abs()), -1).flatten(2)
    shape = (rows // seq_len, seq_len, heads, 128)
    return xs.view(shape).permute(0, 2, 1, 3), terms.view(shape).permute(0, 2, 1, 3)


def head_bound(ref, terms, out_fmt, rope):
    return 0.5 * spacing(ref, out_fmt) + U24 * (K_HEAD_ROPE if rope else K_HEAD_NORM) * terms


def head_check(out, ref, terms, out_fmt, norm, rope, prof, what):
    """out (nseq, heads, seq_len, 128) of the output type.  Normalised: finite, within `head_bound`; not normalised: the fp64 value
    rounded once, bit for bit.  Zero vectors (prof (rows, heads) == 2) give exactly 0.  Returns the worst ratio."""
    assert bool(torch.isfinite(out.float()).all()), f"{what}: output not finite"
    nseq, heads, seq_len, _ = out.shape
    zero = (prof == 2).view(nseq, seq_len, heads).permute(0, 2, 1)
    assert bool((out[zero] == 0).all()), f"{what}: a vector of zeros must give zeros"
    if not norm:
        assert torch.equal(out.double(), rnd(ref, out_fmt)), f"{what}: exact products, one rounding - the output is the rounded fp64 value"
        return 0.0
    return check(out, ref, head_bound(ref, terms, out_fmt, rope), what)


def vt_reference(x, heads, nparts, part, seq_len, sk_pad, perm):
    """The V part as the V^T operand: (nseq, heads, 128, sk_pad), zero pad columns, `perm` = ops.perm16_index(sk_pad)."""
    rows = x.shape[0]
    nseq = rows // seq_len
    v = x.view(nseq, seq_len, heads, nparts, 128)[:, :, :, part].permute(0, 2, 1, 3)
    vpad = torch.zeros((nseq, heads, sk_pad, 128), dtype=x.dtype, device=x.device)
    vpad[:, :, :seq_len] = v
    return vpad[:, :, perm].transpose(-1, -2).contiguous()


# ---- fold preparation --------------------------------------------------------------------------------------------------------------
def fold_operands(N, K, seed, device="cpu"):
    """(W (N, K), gamma (K,), beta (K,), bias (N,)) fp64 of the module docstring."""
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, shape: torch.randint(lo, hi, shape, generator=g).double()
    W = ri(1, 16, (N, K)) * torch.exp2(ri(0, 4, (N, K)) - 6) * (ri(0, 2, (N, K)) * 2 - 1)
    gamma, beta, bias = ri(1, 16, (K,)) / 8, ri(-16, 17, (K,)) / 8, ri(-16, 17, (N,)) / 8
    for fmt in ("bf16", "f16"):
        assert torch.equal(rnd(W, fmt), W) and torch.equal(rnd(W * gamma, fmt), W * gamma), f"W or W gamma is not exact in {fmt}"
    assert float((W * gamma).abs().sum(-1).max()) * 2 ** 9 < 2 ** 24 and float((W * beta).abs().sum(-1).max() + 2) * 2 ** 9 < 2 ** 24
    return tuple(t.to(device) for t in (W, gamma, beta, bias))


def fold_reference(W, gamma, beta, bias):
    wf = W * gamma
    return wf, wf.sum(-1), (W * beta).sum(-1) + (bias if bias is not None else 0.0)


# ---- CPU emulation: the kernels' arithmetic in torch fp32, any summation order ----------------------------------------------------
LN_FAULTS = ("eps_dropped", "eps_1e-6", "eps_outside_root", "var_ex2", "ladder_off_by_one", "c_minus_1", "rounded_twice")
HEAD_FAULTS = ("rms_127", "sine_sign", "frame_off_by_one", "rounded_twice")


def tree_sum(v):
    """Pairwise fp32 sum along the last axis (zero padded to a power of two), as a butterfly adds: one definite order."""
    n = 1 << max(0, (v.shape[-1] - 1).bit_length())
    v = torch.nn.functional.pad(v, (0, n - v.shape[-1]))
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def lane_sum(v, per_lane=8):
    """The row kernels' own order: a lane adds its chunks of `per_lane` columns ((j * 64 + lane) * per_lane + e) one value after the
    other, then the 64 lanes meet in a butterfly."""
    rows, C = v.shape
    nch = -(-C // (64 * per_lane))
    v = torch.nn.functional.pad(v, (0, nch * 64 * per_lane - C)).view(rows, nch, 64, per_lane).permute(0, 2, 1, 3).reshape(rows, 64, -1)
    acc = torch.zeros((rows, 64), dtype=v.dtype)
    for i in range(v.shape[-1]):
        acc = acc + v[..., i]
    return tree_sum(acc)


def _to_out(o, out_fmt, twice=False):
    if twice:                                        # fp32 -> f16 -> bf16: two roundings where the kernel has one
        o = o.to(torch.float16).float()
    return o.to(FORMATS[out_fmt][0])


def emulate_layernorm(x, w, b, eps, out_fmt, fault=None, ladder=LADDER):
    """layernorm_kernel / add_layernorm_f32_kernel (x: the fp32 row values, h + y already added) / layernorm_f32_kernel (out_fmt
    "f32": 1 / sqrt for rsqrt) on the CPU.  Faults: eps dropped; 1e-6 for the eps given; eps added outside the root; the variance as
    E[x^2] - mean^2; C - 1 for C in the variance; the chunk count taken as floor(C / ladder), so that the columns past ladder * NCH
    are neither read nor written (zeros stand for what the output buffer held); the output rounded through f16 first."""
    assert fault is None or fault in LN_FAULTS
    x, w, b = x.float(), w.float().cpu(), b.float().cpu()
    C = x.shape[-1]
    keep = C
    if fault == "ladder_off_by_one":
        nch = max(1, C // ladder)
        keep = min(C, ladder * (1 if nch <= 1 else 2 if nch <= 2 else 4 if nch <= 4 else 8 if nch <= 8 else 16))
    xs = x[:, :keep]
    cf = torch.tensor(float(C), dtype=torch.float32)
    e = torch.tensor({"eps_dropped": 0.0, "eps_1e-6": 1e-6}.get(fault, eps), dtype=torch.float32)
    mean = (tree_sum(xs) / cf)[:, None]
    dl = xs - mean
    if fault == "var_ex2":
        var = lane_sum(xs * xs, 4 if out_fmt == "f32" else 8) / cf - mean[:, 0] * mean[:, 0]
    else:
        var = tree_sum(dl * dl) / (cf - 1 if fault == "c_minus_1" else cf)
    if fault == "eps_outside_root":
        rstd = 1.0 / (torch.sqrt(var) + e)
    else:
        rstd = torch.rsqrt(var + e) if out_fmt != "f32" else 1.0 / torch.sqrt(var + e)
    o = torch.zeros_like(x)
    o[:, :keep] = dl * rstd[:, None] * w[:keep] + b[:keep]
    return _to_out(o, out_fmt, fault == "rounded_twice")


def emulate_row_stats(x, eps):
    """The two-pass statistics of layernorm_kernel (C % 256 != 0) -> (rows, 2) fp32."""
    x = x.float()
    cf = torch.tensor(float(x.shape[-1]), dtype=torch.float32)
    mean = tree_sum(x) / cf
    dl = x - mean[:, None]
    return torch.stack((mean, torch.rsqrt(tree_sum(dl * dl) / cf + torch.tensor(eps, dtype=torch.float32))), -1)


def emulate_head(x, heads, nparts, part, w, rope, seq_len, rpf, out_fmt, eps=HEAD_EPS, fault=None):
    """head_post_kernel's Q / K path on the CPU -> (nseq, heads, seq_len, 128) of the output type.  Faults: 1/127 for RMSNorm's
    1/128; the sine of channel pair 37 negated; the tokens that open a frame rotated by the frame before; the output rounded twice."""
    assert fault is None or fault in HEAD_FAULTS
    rows = x.shape[0]
    v = x.float().view(rows, heads, nparts, 128)[:, :, part]
    if w is not None:
        ss = tree_sum(v * v)
        inv = torch.tensor(1.0 / 127.0 if fault == "rms_127" else 1.0 / 128.0, dtype=torch.float32)
        r = torch.rsqrt(ss * inv + torch.tensor(eps, dtype=torch.float32))
        v = (v * r[..., None]) * w.float().cpu()
    if rope is not None:
        row = torch.arange(rows)
        fr = row // rpf
        if fault == "frame_off_by_one":
            fr = torch.where((row % rpf == 0) & (row > 0), fr - 1, fr)
        cos, sin = (t.float().cpu().clone() for t in rope)
        if fault == "sine_sign":
            sin[:, 37] = -sin[:, 37]
        c, s = cos[fr][:, None, :], sin[fr][:, None, :]
        a, bb = v.reshape(rows, heads, 64, 2).unbind(-1)
        bs, bc = bb * s, bb * c                      # rounded products; the fmas' one rounding through fp64 (the operands are fp32)
        x0 = (a.double() * c.double() - bs.double()).float()
        x1 = (a.double() * s.double() + bc.double()).float()
        v = torch.stack((x0, x1), -1).flatten(2)
    out = _to_out(v, out_fmt, fault == "rounded_twice")
    return out.view(rows // seq_len, seq_len, heads, 128).permute(0, 2, 1, 3)


def emulate_fold(W, gamma, beta, bias, fmt):
    """ln_fold_weight_kernel on the CPU -> (wf of the 16-bit type, colsum, d fp32)."""
    w = W.float()
    wf = (w * gamma.float()).to(FORMATS[fmt][0])
    d = tree_sum(w * beta.float())
    return wf, tree_sum(wf.float()), d + (bias.float() if bias is not None else 0.0)
