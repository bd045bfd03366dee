"""Operands on which am_attention_f32 (csrc/am_f32.hip: attention_f32_kernel) has one correct bit pattern per output element, the
expected bits, a counted bound for the one profile that rounds, a report of the differing elements, and a CPU emulation of the kernel.

The kernel works in natural units with libm expf: p = expf(fmaf(s, scale, -msn)), alpha = expf(ms - msn).  NOTHING is assumed of
the device's expf beyond  expf(0) = 1,  expf(x <= -104) = 0  (e^-104 = 6.9e-46 is under half the smallest fp32 subnormal) and, for
`ladder` alone, the accuracy HIP's published table of device functions states for expf (EXPF_ULPS = 1).  Q and K are integer-valued,
so every score is an exact integer in the fp32 MFMA chain in any order; the keys a query attends to ("members") score exactly 0 and
every other key an integer <= -G with G * float32(scale) >= 110 (asserted), for any scale - the default head_dim ** -0.5 included:
    member      s = 0: msn = 0 * scale = 0, p = expf(0) = 1
    non-member  p = expf(<= -110) = 0 once a member has been seen
    before that the non-members are accumulated with p <= 1 ("junk", finite: asserted) and dropped as a whole by
                alpha = expf(msn_old - 0) = expf(<= -110) = 0 when the first member arrives.
So l is the member count, o the exact sum of the members' V rows, and the output is one IEEE division.  am_f32.hip is built with
FLAGS_am_f32 = -fno-slp-vectorize on top of CXXFLAGS = -O3 (csrc/Makefile): no fast-math flag, and hipcc's fp32 division is
correctly rounded by default (-fhip-fp32-correctly-rounded-divide-sqrt), so the quotient has one admissible bit pattern too.

Profiles (`operands`):
  one_hot       query r attends to exactly one key pi(r): pi(0) = 0, pi(1) = sk - 1 (inside the ragged last block), the rest seeded.
                Head dims in groups of 16: 15 channels carry the key index as +-1 bits (a seeded sign and bit order per group; every
                group carries the whole code), the 16th holds K = 1.  Q of row r is non-zero in ONE group, which rotates with the row:
                c * code(pi(r)) and -15 c, so the score is -2 c hamming(key, pi(r)): 0 for the member, <= -2 c = -G otherwise.
                V: random bits - any sign, exponent within +-100 of 1, any mantissa; never zero.  Expected O[r] == V[pi(r)] bit for bit
                (1 v + 0 rest, then v / 1): every (sequence, head, query, key, channel) index, stride, offset and the tail mask.
  subset        8 classes in groups of 8 channels (a seeded order per group, Q = G in one channel, the group rotating with the row);
                key j holds 0 in the channels of the classes it is a member of and -depth_j (1 here) in the others.  Classes, per
                (sequence, head): 0 members in the first block only, 1 in the last block only, 2 the last key alone, 3 the first key
                alone, 4 half the keys, 5 every key, 6 a power-of-two count, 7 an eighth of the keys.  V = sign_d * m, one seeded sign
                per channel, m in {1..4}.  Expected fl32(sum / count), the correctly rounded quotient of two exact integers < 2^24.
  order_last / order_first / order_rising   the subset operands with every class's members in the last block only / in the first
                block only / in the last block with depth_j falling by one per block: the junk is re-based by >= G at every block
                before the final drop.  Expected as subset.
  plateau       every key a member over 129 blocks (Q in the even channels, K in the odd ones, random small integers: all scores 0).
                l must be exactly sk and every alpha exactly 1.  Expected fl32(sum / sk).
  ladder        the only profile with 0 < alpha < 1: subset's members at scores {0, -1, -2, -3} (Q = 1, K = -level_j, the lowest level
                of a block falling from 3 to 0 along the stream; non-members at -G), scale = 1.0.  Reference: fp64 softmax.
The codes do not depend on the sequence, so the K / V rows of the neighbouring sequences - the rows just past a ragged last block
among them - hold member codes for this sequence's queries: a read across a sequence boundary changes an output bit.

`ladder_bound`, per element relative to |ref| (one sign per channel: no cancellation), counted on attention_f32_kernel in units of
eps = 2^-24, R = 3 the most rises of a running max over four levels, nkb the number of 32-key blocks:
  p and alpha     a key's final weight is one expf for p times one expf per later rise, each EXPF_ULPS 2^-23 = 2 EXPF_ULPS eps,
                  in the numerator and in the row sum                                              2 * 2 EXPF_ULPS (R + 1)   = 16
  l               `bs += p` 16 times, the exchange `bs += __shfl_xor(bs, 32)`, `l = fmaf(l, alpha, bs)` once per block   17 + nkb
  o               the block product: 16 MFMAs of two k-steps each = 32 fmaf steps (a k-ordered fmaf chain, am_f32.hip's header),
                  `o = fmaf(o, alpha, blk)` once per block                                                                32 + nkb
  o / l           one correctly rounded division                                                                                 1
  fmaf(s, 1, -msn), bm * 1.0f                                                                                              exact: 0
x (1 + 2^-10) for the products of the terms.  nkb = 9 at the longest stream (257 keys): 84 eps = 5.0e-6 <= 1e-5 (asserted).
seen: CPU emulation 0.071 of the bound; MI355X 0.071, both builds (ladder-3x2x65x257-d64, row 13, channel 87 on either).

`emulate` restates the kernel's block loop in fp32 torch on the arguments of ops.attention_f32: 32-key blocks, the 16 + 1 row sum in
the kernel's key order (register r of lane half h is key acc_row(r, h)), l = fmaf(l, alpha, bs), a per-block product folded in as
fmaf(o, alpha, blk), the final division; expf and fmaf are computed in fp64 and rounded once.  DEFECTS are planted in it.

What the construction cannot see: a defect whose only effect is a rounding residual of m * scale.  `alpha_unrounded_max` (the defect
the kernel's comment records) makes alpha = expf(m scale - rnd(m scale)); on these operands m scale is 0 or exact, so alpha is 1
either way.  Making it visible needs a member score whose product with scale rounds, and then p = expf(residual) is a fact about expf
near 0 that this file does not assume.  tests/test_attention_f32_exact_cpu.py asserts that blindness next to the defect's rel-L2 on
the randn case, which is what guards it (tests/test_fp32_path_gpu.py, 2e-6)."""
import functools
import math
from typing import NamedTuple, Optional

import torch

AK, AQ = 32, 128                       # keys per block, queries per workgroup
SHAPES = ((1, 1, 1, 1), (2, 3, 33, 31), (2, 3, 129, 33), (1, 2, 300, 97), (3, 2, 65, 257), (2, 3, 97, 97))
PLATEAU_SHAPE = (1, 1, 128, 4113)
HEAD_DIMS = (64, 128)
SCALES = (1.0, 0.125, None)            # None: the default head_dim ** -0.5
BITWISE = ("one_hot", "subset", "order_last", "order_first", "order_rising", "plateau")
PROFILES = BITWISE + ("ladder",)
LAYOUTS = ("plain", "cross", "wide", "mixed", "packed")
NCLASS, OH_W = 8, 16
MIN_GAP = 110.0
EXPF_ULPS = 1.0                        # HIP's published table of device functions: expf, 1 ulp
LADDER_RISES = 3
DEFECTS = ("alpha_unrounded_max", "ms_init_finite", "tail_mask_off_by_one", "bs_exchange_omitted", "kvalid_previous_block",
           "v_row_swapped_halves", "v_head_stride_from_k", "rescale_judged_per_half", "alpha_ulp_every_fourth_block")


class Case(NamedTuple):
    profile: str
    shape: tuple
    D: int
    layout: str
    scale: Optional[float]


def case_id(c):
    return f"{c.profile}-{'x'.join(map(str, c.shape))}-d{c.D}-{c.layout}-s{'dflt' if c.scale is None else c.scale}"


def layouts_for(shape):
    """`packed` is one [q | k | v] tensor: sq == sk only."""
    return LAYOUTS if shape[2] == shape[3] else LAYOUTS[:-1]


def _cases():
    out = []
    for D in HEAD_DIMS:
        for shape in SHAPES:
            for prof in PROFILES:
                if prof == "plateau":
                    continue
                for layout in layouts_for(shape):
                    for scale in ((1.0,) if prof == "ladder" else SCALES):
                        out.append(Case(prof, shape, D, layout, scale))
        for layout in LAYOUTS[:-1]:
            for scale in SCALES:
                out.append(Case("plateau", PLATEAU_SHAPE, D, layout, scale))
    return tuple(out)


CASES = _cases()


def scale_f32(scale, D):
    """The scale the kernel multiplies by: the float32 of what ops.attention_f32 passes."""
    return float(torch.tensor(D ** -0.5 if scale is None else scale, dtype=torch.float32))


def gap(scale, D):
    """G: the smallest integer with G * float32(scale) >= 110, made even (one_hot's scores are multiples of 2 c)."""
    g = math.ceil(MIN_GAP / scale_f32(scale, D))
    return g + (g & 1)


def acc_row(r, h):
    """am_f32.hip: the row of element r of a 32x32 accumulator held by lane half h - here the key (within its block) of register r."""
    return (r & 3) + 8 * (r >> 2) + 4 * h


def key_half(key):
    return (key >> 2) & 1


# ---- operands -------------------------------------------------------------------------------------------------------------------------
def _signs(D, g):
    sign = torch.randint(0, 2, (D,), generator=g) * 2.0 - 1.0
    sign[0], sign[1], sign[4], sign[5] = 1.0, -1.0, -1.0, 1.0        # neither constant over a lane half's four columns nor over halves
    return sign


def _membership(nseq, H, sk, profile, g):
    """bool (nseq, H, sk, NCLASS): the classes key j is a member of (module docstring)."""
    nkb = -(-sk // AK)
    key = torch.arange(sk)
    first, last = key < AK, key >= (nkb - 1) * AK
    u = torch.rand((nseq, H, sk, NCLASS), generator=g)
    mem = torch.zeros((nseq, H, sk, NCLASS), dtype=torch.bool)
    if profile in ("subset", "ladder"):
        mem[..., 0] = (u[..., 0] < 0.5) & first
        mem[:, :, min(5, sk - 1), 0] = True
        mem[..., 1] = (u[..., 1] < 0.5) & last
        mem[:, :, max(sk - 2, (nkb - 1) * AK), 1] = True
        mem[:, :, sk - 1, 2] = True
        mem[:, :, 0, 3] = True
        mem[..., 4] = u[..., 4] < 0.5
        mem[..., 5] = True
        pow2 = 1 << (sk.bit_length() - 1)
        mem[..., 6] = u[..., 6].argsort(-1).argsort(-1) < pow2           # a seeded choice of pow2 keys
        mem[..., 7] = u[..., 7] < 0.125
        forced = torch.randint(0, sk, (nseq, H, 2), generator=g)
        for i, cl in enumerate((4, 7)):
            mem[..., cl].scatter_(-1, forced[..., i:i + 1], True)
    else:
        where = first if profile == "order_first" else last
        mem = (u < 0.4) & where.view(1, 1, sk, 1)
        forced = torch.randint(0, int(where.sum()), (nseq, H, 1, NCLASS), generator=g) + (0 if profile == "order_first" else (nkb - 1) * AK)
        mem.scatter_(2, forced, True)
    return mem


@functools.lru_cache(maxsize=4)
def _base(profile, shape, D):
    """What does not hang on the scale: k, v (nseq, H, sk, D) fp32, the direction of q (its non-zero entries at gap 1) and what the
    profile knows of the answer."""
    nseq, H, sq, sk = shape
    g = torch.Generator().manual_seed(PROFILES.index(profile) * 1000003 + (nseq * 7 + H * 5 + sq * 3 + sk) * 131 + D)
    nkb = -(-sk // AK)
    rows = torch.arange(nseq * H * sq).view(nseq, H, sq)
    info = dict(profile=profile, shape=shape, D=D, pi=None)
    if profile == "one_hot":
        ng = D // OH_W
        sgn = torch.randint(0, 2, (ng, OH_W - 1), generator=g) * 2.0 - 1.0
        order = torch.stack([torch.randperm(OH_W - 1, generator=g) for _ in range(ng)])         # bit carried by channel i of group g
        pi = torch.randint(0, sk, (nseq, H, sq), generator=g)
        pi[:, :, 0] = 0
        if sq > 1:
            pi[:, :, 1] = sk - 1
        code = lambda idx: ((idx.unsqueeze(-1).unsqueeze(-1) >> order) & 1) * 2.0 - 1.0          # (..., ng, 15)
        kc = code(torch.arange(sk)) * sgn                                                       # (sk, ng, 15)
        k = torch.cat([kc, torch.ones((sk, ng, 1))], -1).reshape(sk, D).expand(nseq, H, sk, D).contiguous()
        qc = torch.cat([code(pi) * sgn, torch.full((nseq, H, sq, ng, 1), -(OH_W - 1.0))], -1)   # (nseq, H, sq, ng, 16)
        qdir = (qc * (torch.arange(ng) == (rows % ng).unsqueeze(-1)).unsqueeze(-1)).reshape(nseq, H, sq, D) * 0.5   # gap 1: c = 1/2
        bits = torch.randint(0, 2 ** 23, (nseq, H, sk, D), generator=g, dtype=torch.int32)
        bits |= torch.randint(27, 228, (nseq, H, sk, D), generator=g, dtype=torch.int32) << 23
        bits |= torch.randint(0, 2, (nseq, H, sk, D), generator=g, dtype=torch.int32) << 31
        v = bits.view(torch.float32)
        info["pi"] = pi
    elif profile == "plateau":
        even = (torch.arange(D) % 2 == 0).float()
        qdir = torch.randint(-3, 4, (nseq, H, sq, D), generator=g).float() * even
        k = torch.randint(-3, 4, (nseq, H, sk, D), generator=g).float() * (1 - even)
        v = _signs(D, g) * torch.randint(1, 5, (nseq, H, sk, D), generator=g).float()
    else:
        ng = D // NCLASS
        order = torch.stack([torch.randperm(NCLASS, generator=g) for _ in range(ng)])            # channel of class a in group g
        mem = _membership(nseq, H, sk, profile, g)
        blk = torch.arange(sk) // AK
        if profile == "order_rising":
            depth = (nkb - blk).float()
        else:
            depth = torch.ones(sk)
        if profile == "ladder":
            lo = 3 - torch.clamp((4 * blk) // nkb, max=3)
            span = (4 - lo).float()
            level = lo + (torch.rand((nseq, H, sk), generator=g) * span).floor().clamp(max=3)
            info["level"] = level
            kcls = torch.where(mem, -level.unsqueeze(-1), torch.zeros(()))                        # non-members: - G - level, in operands()
            info["nonmember"] = ~mem
        else:
            kcls = torch.where(mem, torch.zeros(()), -depth.view(1, 1, sk, 1))
        k = kcls[..., order].reshape(nseq, H, sk, D)            # [..., g, i] = kcls[..., order[g, i]]: channel i of group g holds class order[g, i]
        idx = rows % D
        qdir = torch.zeros((nseq, H, sq, D)).scatter_(-1, idx.unsqueeze(-1), 1.0)
        info["cls"] = order[idx // NCLASS, idx % NCLASS]
        info["order"] = order
        v = _signs(D, g) * torch.randint(1, 5, (nseq, H, sk, D), generator=g).float()
    return qdir, k, v, info


def operands(profile, shape, D, scale):
    """fp32 q (nseq, H, sq, D), k, v (nseq, H, sk, D) and a dict of what the profile knows (pi for one_hot).  Checked by `conditions`
    in the tests, not here."""
    assert profile in PROFILES and D in HEAD_DIMS
    qdir, k, v, info = _base(profile, tuple(shape), D)
    G = gap(scale, D)
    info = dict(info, G=G, scale=scale_f32(scale, D))
    if profile == "ladder":
        assert scale == 1.0
        nm = info["nonmember"][..., info["order"]].reshape(k.shape)
        return qdir.clone(), k - G * nm.float(), v, info
    if profile == "plateau":
        return qdir.clone(), k, v, info
    return qdir * G, k, v, info


def scores64(q, k):
    return q.double() @ k.double().transpose(-1, -2)


def conditions(q, k, v, info):
    """What the operands promise, asserted in fp64 on the operands alone.  Returns the member mask (nseq, H, sq, sk)."""
    profile, (nseq, H, sq, sk), D, G, scale = info["profile"], info["shape"], info["D"], info["G"], info["scale"]
    nkb = -(-sk // AK)
    for t in (q, k):
        assert bool((t == t.round()).all()), "Q or K is not integer-valued"
    s = scores64(q, k)
    assert bool((s == s.round()).all()) and float(s.abs().max()) < 2 ** 24, "a score is not an exact fp32 integer"
    assert float((q.double().abs() @ k.double().abs().transpose(-1, -2)).max()) < 2 ** 24, "a partial score sum can round"
    assert G * scale >= MIN_GAP, f"gap {G} x scale {scale} < {MIN_GAP}"
    top = 0.0
    mem = s >= -3.0 if profile == "ladder" else s == top
    assert bool((s.amax(-1) == top).all()) or profile == "ladder", "a query whose best score is not 0"
    assert bool(mem.any(-1).all()), "a query without a member"
    assert bool((s[~mem] <= -G).all()), "a non-member above -G"
    rows = nseq * H * sq
    if profile != "plateau" and rows >= D:
        assert bool((q != 0).flatten(0, 2).any(0).all()), "a head dim that no query uses"
    blk = torch.arange(sk) // AK
    hit = torch.zeros(nkb, dtype=torch.bool)
    hit[blk[mem.flatten(0, 2).any(0)]] = True
    if profile in ("one_hot", "subset", "ladder", "plateau") and rows >= 2 * nkb:
        assert bool(hit.all()), "a key block that holds no query's member"
    vmax = float(v.double().abs().max())
    assert math.isfinite(vmax) and sk * vmax < 3.0e38, "the junk can overflow"
    if profile == "one_hot":
        pi = info["pi"]
        assert bool((mem.sum(-1) == 1).all()) and bool(mem.gather(-1, pi.unsqueeze(-1)).all()), "one_hot: the member is not pi(r) alone"
        assert bool((pi[:, :, 0] == 0).all()) and (sq == 1 or bool((pi[:, :, 1] == sk - 1).all()))
        e = (v.view(torch.int32) >> 23) & 0xFF
        assert int(e.min()) >= 27 and int(e.max()) <= 227, "one_hot: a V exponent outside +-100"
        if rows >= 64 and sk >= 8:
            assert len(set(key_half(pi.flatten() % AK).tolist())) == 2, "one_hot: a lane half that holds no member"
    else:
        assert bool((v == v.round()).all()) and float(v.abs().min()) >= 1 and float(v.abs().max()) <= 4
        assert bool(((v > 0).flatten(0, 2).all(0) | (v < 0).flatten(0, 2).all(0)).all()), "a channel with both signs"
        assert 4 * sk < 2 ** 24, "a member sum can round"
    if profile in ("subset", "ladder"):
        cnt = mem.sum(-1)
        cls = info["cls"]
        assert bool((cnt[cls == 2] == 1).all()) and bool(mem[..., sk - 1][cls == 2].all()), "class 2 is not the last key alone"
        assert bool((cnt[cls == 5] == sk).all())
        if nkb > 1:
            assert bool((~mem[..., AK:].any(-1))[cls == 0].all()) and bool((~mem[..., :(nkb - 1) * AK].any(-1))[cls == 1].all())
    if profile.startswith("order") and nkb > 1:
        inside = blk == (0 if profile == "order_first" else nkb - 1)
        assert not bool(mem[..., ~inside].any()), f"{profile}: a member outside its block"
        if profile == "order_rising":
            bmax = torch.stack([s[..., blk == b].amax(-1) for b in range(nkb)], -1)
            assert bool((bmax.diff(dim=-1) >= G).all()), "order_rising: a block that does not rise by G"
    if profile == "plateau":
        assert bool(mem.all())
    if profile == "ladder":
        assert nkb <= 9 and ladder_bound(nkb) <= 1e-5, "ladder: the stream is too long for its bound"
    return mem


def expected(q, k, v, info, mem):
    """(nseq * sq, H * D): fp32 whose bits are the answer (BITWISE profiles), or the fp64 softmax (ladder)."""
    nseq, H, sq, sk = info["shape"]
    if info["profile"] == "ladder":
        p = torch.softmax(scores64(q, k) * info["scale"], -1)
        out = p @ v.double()
    elif info["profile"] == "one_hot":
        out = v.gather(2, info["pi"].unsqueeze(-1).expand(-1, -1, -1, info["D"]))
    else:
        total, cnt = mem.double() @ v.double(), mem.sum(-1, keepdim=True).double()
        assert float(total.abs().max()) < 2 ** 24
        out = total.float() / cnt.float()                        # IEEE: the correctly rounded quotient of two exact fp32 integers
        assert torch.equal(out, (total / cnt).float())
    return out.transpose(1, 2).reshape(nseq * sq, H * info["D"])


def ladder_bound(nkb):
    """Relative ceiling of |out - ref| / |ref| for `ladder` (module docstring), counted, not fitted."""
    units = 2 * 2 * EXPF_ULPS * (LADDER_RISES + 1) + (17 + nkb) + (32 + nkb) + 1
    return units * 2.0 ** -24 * (1 + 2.0 ** -10)


def ladder_ratio(out, ref, nkb, what):
    """max |out - ref| / (ladder_bound |ref|), printed; |ref| >= 1 (one sign per channel, |v| >= 1)."""
    r = (out.double().cpu() - ref).abs() / (ladder_bound(nkb) * ref.abs())
    r = torch.where(torch.isfinite(out.double().cpu()), r, torch.full_like(r, float("inf")))
    at = int(r.argmax())
    row, ch = divmod(at, ref.shape[1])
    worst = float(r.flatten()[at])
    print(f"exact-f32 attention {what}: max err / bound {worst:.3f} at (row {row}, channel {ch})")
    return worst


def mismatch_report(out, want, info, mem=None, what=""):
    """None when out and want agree bit for bit; else the text of the assertion: how many elements differ, the first few, and the
    residues that hold them - sequence, head, query (mod 128: the workgroup's row, / 32 its wave), key block of the query's first
    member, lane half h and register group of the channel, channel."""
    nseq, H, sq, sk = info["shape"]
    D = info["D"]
    out, want = out.cpu().contiguous(), want.cpu().contiguous()
    assert out.shape == want.shape == (nseq * sq, H * D) and out.dtype == want.dtype == torch.float32
    bad = out.view(torch.int32) != want.view(torch.int32)
    if not bool(bad.any()):
        return None
    rows, cols = bad.nonzero(as_tuple=True)
    seq, qi, head, ch = rows // sq, rows % sq, cols // D, cols % D
    ulps = (out.view(torch.int32)[rows, cols].long() - want.view(torch.int32)[rows, cols].long()).abs()
    lines = [f"{what}: {int(bad.sum())} of {bad.numel()} elements differ ({int((~torch.isfinite(out)).sum())} not finite); "
             f"bit patterns apart: min {int(ulps.min())}, max {int(ulps.max())}"]
    for i in range(min(6, rows.numel())):
        r, c = int(rows[i]), int(cols[i])
        lines.append(f"  (seq {int(seq[i])}, head {int(head[i])}, query {int(qi[i])}, channel {int(ch[i])}): got {float(out[r, c])!r}, want {float(want[r, c])!r}")

    def res(name, x):
        u = sorted(set(x.tolist()))
        return f"{name} {u if len(u) <= 16 else f'{len(u)} values, {u[0]} .. {u[-1]}'}"
    parts = [res("seq", seq), res("head", head), res("query % 128", qi % AQ), res("wave", (qi % AQ) // 32), res("lane half h", key_half(ch)),
             res("channel % 32", ch % 32), res("channel // 32", ch // 32)]
    if mem is not None:
        first = mem.float().argmax(-1)[seq, head, qi]
        cnt = mem.sum(-1)[seq, head, qi]
        parts += [res("first member's block", first // AK), res("its lane half", key_half(first % AK)), res("member count", cnt)]
    lines.append("  " + "; ".join(parts))
    return "\n".join(lines)


# ---- layouts ---------------------------------------------------------------------------------------------------------------------------
def place(q, k, v, layout, make):
    """The 2-D operands and keyword arguments of ops.attention_f32 for `layout`.  make(t2d) -> a 2-D tensor holding t2d (the GPU tests
    give an arena with poisoned gaps and guards; the CPU tests the tensor itself).  NaN fills every column no head owns.
      plain   q, k, v (rows, H D) each        cross   kv (rows, 2 H D): head h is [k_h | v_h], k_hs = v_hs = 2 D, v_off = D
      wide    plain; the test gives an out wider than H D
      mixed   k inside a per-head [k_h | NaN] tensor (k_hs = 2 D), v plain (v_hs = D): the two head strides differ
      packed  [4 NaN | q | 4 NaN | k | 4 NaN | v | 4 NaN]: column offsets 4, H D + 8, 2 H D + 12"""
    nseq, H, sq, D = q.shape
    sk = k.shape[2]
    flat = lambda t: t.transpose(1, 2).reshape(nseq * t.shape[2], H * D)
    nan = float("nan")
    if layout in ("plain", "wide"):
        return make(flat(q)), make(flat(k)), make(flat(v)), {}
    if layout == "cross":
        kv = torch.stack([k.transpose(1, 2), v.transpose(1, 2)], 3).reshape(nseq * sk, 2 * H * D)
        kv = make(kv)
        return make(flat(q)), kv, kv, dict(k_hs=2 * D, v_hs=2 * D, v_off=D)
    if layout == "mixed":
        kx = torch.stack([k.transpose(1, 2), torch.full_like(k.transpose(1, 2), nan)], 3).reshape(nseq * sk, 2 * H * D)
        return make(flat(q)), make(kx), make(flat(v)), dict(k_hs=2 * D)
    assert layout == "packed" and sq == sk
    pad = torch.full((nseq * sq, 4), nan)
    qkv = make(torch.cat([pad, flat(q), pad, flat(k), pad, flat(v), pad], 1))
    return qkv, qkv, qkv, dict(q_off=4, k_off=H * D + 8, v_off=2 * H * D + 12)


# ---- CPU emulation of attention_f32_kernel ------------------------------------------------------------------------------------------------
def _expf(x):
    return torch.exp(x.double()).float()


def _fmaf(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def _heads(t, nseq, n, H, D, off, hs):
    """The kernel's addressing: head h of row r is t[r, off + h hs : + D] -> (nseq * H, n, D); NaN where that leaves the row."""
    cols = off + hs * torch.arange(H).view(H, 1) + torch.arange(D)
    ok = cols < t.shape[1]
    x = t[:, cols.clamp(max=t.shape[1] - 1)]
    x = torch.where(ok, x, torch.full((), float("nan")))
    return x.view(nseq, n, H, D).transpose(1, 2).reshape(nseq * H, n, D)


def emulate(q, k, v, heads, sq, sk, D, q_hs=None, k_hs=None, v_hs=None, q_off=0, k_off=0, v_off=0, scale=None, defect=None):
    """attention_f32_kernel on the CPU, on the arguments of ops.attention_f32 -> (nseq * sq, heads * D) fp32 (module docstring).
    The scores are one fp64 product rounded to fp32 (exact on integer operands).  defect, one of DEFECTS:
      alpha_unrounded_max      alpha = expf(fmaf(m_old, scale, -msn)), m_old the unscaled running max (the kernel's comment)
      ms_init_finite           ms starts at -87 (expf(-87) is still a normal number) instead of -inf
      tail_mask_off_by_one     `acc_row(r, h) > kvalid`: the first key past sk (a zero row of the loader) is kept
      bs_exchange_omitted      block min(1, nkb - 1) adds only the lane half's own 16 keys to l
      kvalid_previous_block    kvalid = sk - (kb - 1) 32: the tail is never masked
      v_row_swapped_halves     P.V pairs the probability of key acc_row(s, h) with the V row of key acc_row(s, 1 - h)
      v_head_stride_from_k     V's head h read at v_off + h k_hs
      rescale_judged_per_half  o is rescaled only where the lane half's OWN 16 keys raise the max (judged before the exchange)
      alpha_ulp_every_fourth_block   alpha = 1 + 2^-23 where it should be 1, on every fourth block: a quarter of the drift the kernel's comment records"""
    assert defect is None or defect in DEFECTS
    nseq = q.shape[0] // sq
    q_hs, k_hs, v_hs = (D if x is None else x for x in (q_hs, k_hs, v_hs))
    if defect == "v_head_stride_from_k":
        v_hs = k_hs
    sc = torch.tensor(D ** -0.5 if scale is None else scale, dtype=torch.float32)
    qh, kh, vh = _heads(q, nseq, sq, heads, D, q_off, q_hs), _heads(k, nseq, sk, heads, D, k_off, k_hs), _heads(v, nseq, sk, heads, D, v_off, v_hs)
    B = nseq * heads
    half = key_half(torch.arange(AK))                                   # lane half of a key of the block
    chalf = key_half(torch.arange(D))                                   # lane half that holds an output channel
    o = torch.zeros((B, sq, D))
    l = torch.zeros((B, sq, 2))
    ms = torch.full((B, sq), -87.0 if defect == "ms_init_finite" else float("-inf"))
    mraw = torch.full((B, sq), float("-inf"))
    nkb = -(-sk // AK)
    for kb in range(nkb):
        n = min(AK, sk - kb * AK)
        kblk, vblk = torch.zeros((B, AK, D)), torch.zeros((B, AK, D))   # the loader's zero rows past sk
        kblk[:, :n], vblk[:, :n] = kh[:, kb * AK:kb * AK + n], vh[:, kb * AK:kb * AK + n]
        s = (qh.double() @ kblk.double().transpose(-1, -2)).float()
        kvalid = sk - kb * AK
        if defect == "kvalid_previous_block":
            kvalid += AK
        if defect == "tail_mask_off_by_one":
            kvalid += 1
        s[..., torch.arange(AK) >= kvalid] = float("-inf")
        bm_h = torch.stack([s[..., half == 0].amax(-1), s[..., half == 1].amax(-1)], -1)
        bm = bm_h.amax(-1)
        msn = torch.maximum(ms, bm * sc)
        alpha = _expf(ms - msn)
        if defect == "alpha_unrounded_max":
            alpha = _expf(_fmaf(mraw, sc, -msn))
            mraw = torch.maximum(mraw, bm)
        if defect == "alpha_ulp_every_fourth_block" and kb % 4 == 3:
            alpha = torch.where(alpha == 1, torch.tensor(1.0 + 2.0 ** -23), alpha)
        p = _expf(_fmaf(s, sc, -msn.unsqueeze(-1)))
        bs_h = torch.zeros((B, sq, 2))
        for r in range(16):
            for h in range(2):
                bs_h[..., h] = bs_h[..., h] + p[..., acc_row(r, h)]
        bs = (bs_h[..., 0] + bs_h[..., 1]).unsqueeze(-1).expand(-1, -1, 2)
        if defect == "bs_exchange_omitted" and kb == min(1, nkb - 1):
            bs = bs_h
        l = _fmaf(l, alpha.unsqueeze(-1), bs)
        blk = torch.zeros((B, sq, D))
        for st in range(16):
            for h in range(2):
                key = acc_row(st, h)
                vkey = acc_row(st, 1 - h) if defect == "v_row_swapped_halves" else key
                blk = _fmaf(vblk[:, vkey].unsqueeze(1), p[..., key].unsqueeze(-1), blk)
        a_o = alpha.unsqueeze(-1).expand(-1, -1, D)
        if defect == "rescale_judged_per_half":
            rises = (bm_h * sc > ms.unsqueeze(-1))[..., chalf]
            a_o = torch.where(rises, a_o, torch.ones(()))
        o = _fmaf(o, a_o, blk)
        ms = msn
    out = o / l[..., chalf]
    return out.view(nseq, heads, sq, D).transpose(1, 2).reshape(nseq * sq, heads * D)
