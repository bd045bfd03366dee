"""Attention operands on which the softmax is exact, an fp64 reference, a componentwise bound, and a CPU emulation of the kernels.

Every attention kernel forms c = scale * 1.4426950408889634f in fp32 and works in log2 units.  With scale = SCALE = float32(ln 2)
that product is exactly 1.0f, so Q' = Q and the softmax is base 2.  With integer-valued Q and K every score is an integer, every
probability 2^(s - m_run [+ 5]) a power of two - exact in bf16, f16 and e4m3 (in the exponent-field form of fp8 too: 2^n (1 + f) at
f = 0) - and small integers are exact in all three operand formats, so the fp8 quantiser is the identity.  What is left of a kernel's
error is its fp32 accumulation and the one rounding of the output: `bound` is that, per element, with no fitted constant.

Operands (`operands`), head width 128:
  Q   two +-1 entries per row whose positions rotate with the row index (every dim but the two reserved ones is met), + 1 in the
      stair dim.  One row in 23 is "flat": a single 1 in the dim where every key holds 1 - all its scores are equal.
  K   entries in {-1, 0, 1}; 1 in the flat rows' dim; the stair dim carries an integer offset that is constant over stretches of keys.
      A score is (a sum of two entries of {-1, 0, 1}) + the key's stair level: within 4 of the top of its level.
  V   sign_d * m: a seeded random sign per channel, m in {1..4} per key and channel.  One sign per channel means no cancellation:
      sum_j p_j |v_jd| / l = |ref_d|, so an absolute rounding bound on the two sums is a RELATIVE bound on the element.
Profiles of the stair:
  window      no stair: every key within 4 of its row's max, every tile matters.
  stair_up    the running max rises along the key stream.  The last few keys stand `step` above the running max before them
              (asserted): 4 for the fp8 kernels (deferred threshold 2^3), 9 for the 16-bit kernels (2^8) - the one re-base a deferred
              kernel cannot put off.  Their other entries are 0, so each scores exactly its level, and they are few, so that the
              keys BEFORE the step keep a tenth of the row sum or more (asserted in fp64): a wrong rescale of what was accumulated
              so far shows.  The 16-bit family also rises by 1 at mid-stream, a step under every threshold, where the stream is long
              enough (1024 keys) to keep that tenth with the first half one octave lower.  A one-tile stream has no stair.
  stair_down  the row max stands in the first tile, later tiles lie 1..4 lower.
Two families (FAMILY): the kernels' thresholds differ, and so does what keeps their probabilities exact.  "fp8": every score within 8
of its row's max, so p >= 2^-8 2^5 = 2^-3 in e4m3 whatever m_run the kernel holds and in whatever order it walks the chunks (e4m3 is
normal down to 2^-6).  "16bit": within 14, so p >= 2^-14 stays a normal number in f16 (bf16 has fp32's range), again for any order;
these operands are never given to an fp8 kernel.  In the natural order no key lies more than 8 below the running max of the tiles
up to and including its own - except, in the 16-bit family, the keys that share a tile with the 9-step (13 below).
All of this is asserted on the operands alone, against fp64, before any kernel sees them.

Unforeseen rounding sites (a form whose bound carries an `extra` term): none."""
import torch

SCALE = 0.6931471824645996          # float32(ln 2): float32(SCALE) * float32(log2 e) == 1.0f
LOG2E_F32 = 1.4426950408889634      # the literal of the kernels
D = 128
TILE = 64
D_STAIR, D_ONE = 77, 41             # reserved dims: the stair level of a key; 1 on every key (the flat rows' dim)
FLAT_EVERY, FLAT_AT = 23, 11        # row r (counted over sequences and heads) is flat when r % 23 == 11
PROFILES = ("window", "stair_up", "stair_down")
FAMILY = {"fp8": dict(step=4, spread=8, tile_below=8), "16bit": dict(step=9, spread=14, tile_below=13)}
FORMATS = {"bf16": torch.bfloat16, "f16": torch.float16, "e4m3": torch.float8_e4m3fn}
U_OUT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}      # unit roundoff of the output


def _round(x, fmt):
    return x.to(FORMATS[fmt]).to(x.dtype)


def key_tiles(sk_total, nchunks):
    """Tile index (in stream order) of every key: chunks of sk_total / nchunks keys, each cut into 64-key tiles of its own."""
    skc = sk_total // nchunks
    tiles_c = -(-skc // TILE)
    key = torch.arange(sk_total)
    return (key // skc) * tiles_c + (key % skc) // TILE, nchunks * tiles_c


def operands(nseq, H, sq, sk_total, profile, seed, family="16bit", nchunks=1, device="cpu"):
    """Integer-valued fp32 q (nseq, H, sq, 128), k, v (nseq, H, sk_total, 128) of `profile` (module docstring), on `device`, checked
    by `conditions`.  `nchunks`: the equal key chunks the stream is laid out in (each is cut into 64-key tiles of its own)."""
    assert profile in PROFILES and family in FAMILY and sk_total % nchunks == 0
    fam = FAMILY[family]
    g = torch.Generator().manual_seed(seed)
    tile, n_tiles = key_tiles(sk_total, nchunks)

    rr = torch.arange(nseq * H * sq).view(nseq, H, sq)
    flat = rr % FLAT_EVERY == FLAT_AT
    free = torch.tensor([d for d in range(D) if d not in (D_STAIR, D_ONE)])
    q = torch.zeros((nseq, H, sq, D))
    for i in range(2):
        sgn = torch.randint(0, 2, rr.shape, generator=g) * 2.0 - 1.0
        q.scatter_(-1, free[(rr + 63 * i) % 126].unsqueeze(-1), sgn.unsqueeze(-1))
    q[..., D_STAIR] = 1.0
    q[flat] = 0.0
    q[..., D_ONE] = flat.float()
    if nseq * H * sq >= 126:
        assert bool((q.abs().amax((0, 1, 2)) == 1).all()), "a head dim that no query row uses"

    stair = torch.zeros(sk_total)
    step_at = None
    if profile == "stair_up" and n_tiles > 1:
        level, before = 0.0, 12.25 / 9.0                         # E 2^(a + b), a and b uniform in {-1, 0, 1}
        if fam["spread"] - 4 - fam["step"] >= 1 and sk_total >= 1024:     # room for a step under the threshold
            stair[tile >= n_tiles // 2] = 1.0
            level, before = 1.0, before * 1.5
        top = level + 2.0 + fam["step"]                          # the running max stands at level + 2 when the step comes
        after = max(1, round(sk_total / (1.0 + 2.0 ** top / before)))     # as many keys as carry half of the row sum
        step_at = sk_total - after
        stair[step_at:] = top
    elif profile == "stair_down":
        stair = torch.where(tile == 0, 0.0, -(1.0 + (tile - 1) % 4))
    k = torch.randint(-1, 2, (nseq, H, sk_total, D), generator=g).float()
    if step_at is not None:
        k[:, :, step_at:] = 0.0                                  # the keys behind the step score exactly their level
    k[..., D_ONE] = 1.0
    k[..., D_STAIR] = stair

    sign = torch.randint(0, 2, (D,), generator=g) * 2.0 - 1.0
    for grp in (2, 4, 8, 16):                                    # not a pattern of 2 / 4 / 8 / 16-lane groups
        rows = sign.view(-1, grp)
        assert not bool((rows == rows[:1]).all()) and not bool((rows == rows[:, :1]).all()), f"channel signs repeat in groups of {grp}"
    v = sign * torch.randint(1, 5, (nseq, H, sk_total, D), generator=g).float()

    q, k, v = q.to(device), k.to(device), v.to(device)
    conditions(q, k, v, profile, family, nchunks, step_at)
    return q, k, v


def round_trips(*tensors):
    """Every operand survives bf16, f16 and e4m3 bit for bit."""
    for t in tensors:
        for name, fmt in FORMATS.items():
            assert torch.equal(t.to(fmt).to(torch.float32), t), f"an operand does not round-trip through {name}"


def _scores(q, k):
    """fp64 scores in log2 units (scale * log2 e = 1)."""
    return q.double() @ k.double().transpose(-1, -2)


def conditions(q, k, v, profile, family, nchunks=1, step_at=None):
    """What the operands promise (module docstring), asserted against fp64 scores; one sequence at a time to bound the memory.
    Returns the facts it measured."""
    fam = FAMILY[family]
    round_trips(q, k, v)
    nseq, H, sq, _ = q.shape
    sk_total = k.shape[2]
    tile, n_tiles = key_tiles(sk_total, nchunks)
    tile = tile.to(q.device)
    facts = dict(spread=0.0, tile_below=0.0, before_share=1.0, flat_rows=0)
    for n in range(nseq):
        s = _scores(q[n], k[n])                                               # (H, sq, sk_total)
        assert bool((s == s.round()).all()), "a score is not an integer"
        top = s.amax(-1)
        facts["spread"] = max(facts["spread"], float((top - s.amin(-1)).max()))
        idx = tile.expand(H, sq, sk_total)
        tmax = torch.full((H, sq, n_tiles), float("-inf"), dtype=s.dtype, device=s.device).scatter_reduce(-1, idx, s, "amax")
        run = tmax.cummax(-1).values.gather(-1, idx)                          # running max of the tiles up to and including the key's
        facts["tile_below"] = max(facts["tile_below"], float((run - s).max()))
        flat = q[n, :, :, D_ONE] == 1
        facts["flat_rows"] += int(flat.sum())
        assert bool(((top - s.amin(-1))[flat] == 0).all()), "a flat row with unequal scores"
        if step_at is not None:
            w = torch.exp2(s - top.unsqueeze(-1))
            share = w[..., :step_at].sum(-1) / w.sum(-1)
            facts["before_share"] = min(facts["before_share"], float(share[~flat].min()))
            rise = (s[..., step_at:].amin(-1) - s[..., :step_at].amax(-1))[~flat]
            assert float(rise.min()) >= fam["step"] and float(rise.median()) == fam["step"], "the step is not the family's"
        if profile == "stair_down" and n_tiles > 1:
            assert bool((tmax[..., 0] == top)[~flat].all()), "stair_down: a row whose max is not in the first tile"
    assert facts["spread"] <= fam["spread"], f"a key {facts['spread']} below its row's max (family {family}: {fam['spread']})"
    assert facts["tile_below"] <= fam["tile_below"], f"a key {facts['tile_below']} below the running max of its tile"
    assert step_at is None or facts["before_share"] >= 0.10, f"the keys before the step carry {facts['before_share']:.3f} of a row sum"
    assert nseq * H * sq < FLAT_EVERY or facts["flat_rows"] > 0
    return facts


def reference(q, k, v):
    """fp64 base-2 softmax attention: p = exp2(s - max s), o = p v / sum p  ->  (nseq * sq, H * 128)."""
    nseq, H, sq, d = q.shape
    out = torch.empty((nseq, sq, H, d), dtype=torch.float64, device=q.device)
    for n in range(nseq):
        s = _scores(q[n], k[n])
        p = torch.exp2(s - s.amax(-1, keepdim=True))
        out[n] = ((p @ v[n].double()) / p.sum(-1, keepdim=True)).transpose(0, 1)
    return out.reshape(nseq * sq, H * d)


def bound(ref, n_keys, out_dtype, extra=0.0):
    """Per-element ceiling of |out - ref|: (u_out + 4 n_keys 2^-24 [+ extra]) |ref|.  u_out: the one rounding of the output (2^-8
    bf16, 2^-11 f16).  n_keys 2^-24 each for the numerator and the row sum added in any order with round-to-nearest (gamma_n, relative
    to sum |terms| = the sum itself: one sign per channel), doubled because the MFMA's internal adder may truncate.  `extra`: the unit
    roundoff of a rounding site named in the module docstring, never a fitted factor."""
    return (U_OUT[out_dtype] + 4.0 * n_keys * 2.0 ** -24 + extra) * ref.abs()


def ratio(out, ref, bnd, what):
    """max |out - ref| / bound, printed with its (row, channel); 0 / 0 (ref = 0 cannot happen: |v| >= 1) counts as 0."""
    err = (out.double() - ref).abs()
    r = torch.where(bnd > 0, err / bnd, err * float("inf")).nan_to_num(nan=0.0, posinf=float("inf"))
    at = int(r.argmax())
    row, ch = divmod(at, ref.shape[1])
    worst = float(r.flatten()[at])
    print(f"exact-softmax {what}: max err / bound {worst:.3f} at (row {row}, channel {ch})")
    return worst, row, ch


def check(out, ref, n_keys, what, extra=0.0):
    """Every element finite and within `bound`; returns the max ratio."""
    assert bool(torch.isfinite(out.float()).all()), f"{what}: output not finite"
    worst, row, ch = ratio(out, ref, bound(ref, n_keys, out.dtype, extra), what)
    assert worst <= 1.0, (f"{what}: |out - ref| = {worst:.3f} x bound at (row {row}, channel {ch}): out {float(out[row, ch])!r}, "
                          f"ref {float(ref[row, ch])!r}")
    return worst


# ---- CPU emulation of the kernels' online softmax -------------------------------------------------------------------------------
def fault_site(q, k, v):
    """(sequence * H + head, row, key, weight): the key whose fp64 softmax weight is the smallest one at or above 5 % of its row."""
    w = torch.softmax(_scores(q, k).flatten(0, 1) * SCALE, -1)
    assert float(w.max()) >= 0.05, "no key carries 5 % of its row"
    at = int(torch.where(w >= 0.05, w, torch.full_like(w, 2.0)).argmin())
    b, rem = divmod(at, w.shape[1] * w.shape[2])
    row, key = divmod(rem, w.shape[2])
    return b, row, key, float(w[b, row, key])


def emulate(q, k, v, p_format, out_format, defer, shift, fault=None):
    """The kernels' arithmetic in torch on the CPU, one chunk: 64-key tiles, fp32 O and l, m_run set by the first tile and re-based
    (per row) only when a tile's max stands more than `defer` above it, p = 2^(s - m_run + shift) rounded to `p_format` for P.V and
    unrounded in the row sum, O / l rounded to `out_format`.  -> fp32 (nseq * sq, H * 128).
    fault (at `fault_site`): "p_off" that probability x (1 + 2^-3); "l_miss" that key left out of the row sum; "alpha" the rescale of
    that row at the re-base in that key's tile doubled."""
    assert fault in (None, "p_off", "l_miss", "alpha")
    nseq, H, sq, d = q.shape
    sk = k.shape[2]
    qf, kf, vf = (t.float().flatten(0, 1) for t in (q, k, v))
    c = torch.tensor(SCALE, dtype=torch.float32) * torch.tensor(LOG2E_F32, dtype=torch.float32)
    qf = _round(qf * c, p_format)                                   # the kernels re-round the pre-scaled Q to the operand format
    fb, frow, fkey, _ = fault_site(q, k, v) if fault else (0, 0, -1, 0.0)
    O = torch.zeros((nseq * H, sq, d))
    l = torch.zeros((nseq * H, sq))
    m = torch.zeros((nseq * H, sq))
    hit = False
    for t0 in range(0, sk, TILE):
        s = qf @ kf[:, t0:t0 + TILE].transpose(-1, -2)
        mx = s.amax(-1) - m
        if t0 == 0:
            m = m + mx
        else:
            delta = torch.where(mx > defer, mx, torch.zeros_like(mx))
            alpha = torch.exp2(-delta)
            if fault == "alpha" and t0 <= fkey < t0 + TILE:
                assert float(delta[fb, frow]) > 0, "the faulted key's tile does not re-base its row"
                alpha[fb, frow] *= 2.0
                hit = True
            m, l, O = m + delta, l * alpha, O * alpha.unsqueeze(-1)
        p = torch.exp2(s - m.unsqueeze(-1) + shift)
        here = fault in ("p_off", "l_miss") and t0 <= fkey < t0 + TILE
        if here and fault == "p_off":
            p[fb, frow, fkey - t0] *= 1.0 + 2.0 ** -3
        rs = p.sum(-1)
        if here and fault == "l_miss":
            rs[fb, frow] -= p[fb, frow, fkey - t0]
        hit = hit or here
        l = l + rs
        O = O + _round(p, p_format) @ vf[:, t0:t0 + TILE]
    assert fault is None or hit
    out = _round(O / l.unsqueeze(-1), out_format)
    return out.view(nseq, H, sq, d).permute(0, 2, 1, 3).reshape(nseq * sq, H * d)
