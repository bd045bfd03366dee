"""fp8 attention where its probabilities leave e4m3's range: one dominant key G octaves above a long tail, and an fp64 emulation of what
each dispatch form of actionmesh_amd/csrc/am_attention_fp8.hip does with the tail.

The kernels carry p = 2^(s - m_run + 5) and pack it to e4m3 (smallest subnormal 2^-9, round to nearest even) for the P.V MFMA.  A key
that is exponentiated against a running maximum 15 or more octaves above it contributes nothing to the numerator (2^-10 is the tie
between 0 and 2^-9 and goes to the even neighbour, 0).  What the ROW SUM does with such a key depends on the kernel (KERNELS), and
whether a key is exponentiated against the final maximum at all depends on WHEN it is seen: a tile walked before the dominant key
arrives is packed at 2^5 and rescaled in fp32 afterwards, so it is never flushed.  `emulate` walks the 64-key tiles in the order the
form walks them and is the reference of tests/test_fp8_range_gpu.py; tests/test_fp8_range_cpu.py holds it against the plain fp64
softmax inside the range, against the table at the edges, and shows that a wrong convention would not pass.

Case (`case`, after _peaky_case of tests/test_f16_kernels_gpu.py): Q = e0 on every row, scale = _attention_exact.SCALE (the product
scale * log2 e is exactly 1.0f), so the score of a key is its K[.., 0] in the kernels' log2 units.  One dominant key G e0; the tail
  pow2     K = 0: every tail score is 0 and every probability a power of two;
  eighths  tail key j of a chunk scores -(j mod 8) / 8 (multiples of 1/8 down to -7/8 have at most three significant bits: exact in
           e4m3, on the same channel).  In the fast form the byte 96 - 8 G - (j mod 8) is an exact integer; in the exp2 forms the
           rounding of 2^(5 - G - f) to e4m3 is deterministic as long as no such value lies near a tie (`tie_distance`, asserted).
V is the indicator of the key's tile (channel = tile mod 128) on the tail and 1 + (c mod 8) / 8 in channel c on the dominant key -
_peaky_case's 1 + c / 128 needs seven mantissa bits and the fp8 quantiser must stay the identity - or 1 everywhere (the twin).
Every sequence and head carries the same operands, and every query row the same scores: the expected output is one vector per class
of rows (the rows of the main grid; the rows of a short last block, which always run the 8-wave kernel)."""
from collections import namedtuple

import torch

import _attention_exact as X

TILE = X.TILE
P_SHIFT, DEFER = 5.0, 3.0                # p = 2^(s - m_run + 5); a tile re-bases m_run when its max stands more than 2^3 above it
SPLIT_Z = 16                             # cuts of a split last block (AM_ATTN_SPLIT_Z)
FORMS = (0, 100, 200, 400)               # `ablate` of ops.attention_fp8: product dispatch, 4 waves x 64 rows, 8-wave, fp8_fast
PROFILES = ("pow2", "eighths")
WHERE = ("first", "middle", "last")

# kernel: (how a probability is formed, which probabilities the row sum adds, where am_attention_fp8.hip says so)
KERNELS = {
    "wave8": ("exp2", "unrounded", "attn_fp8_kernel, softmax(): `ps2[0] += f32x2_t{e[0], e[1]}` adds the v_exp_f32 results; the "
                                   "v_cvt_pk_fp8_f32 of the same e[] comes after it"),
    "x64": ("exp2", "unrounded", "XExpSumPack::step: XES_AD adds get(sa, sb, a), the exponential left by XES_EX; XES_PK packs it a round later"),
    "product": ("exp2", "rounded", "attn_fp8p_kernel, j4: `mfma_f8_acc(lacc, fb, pc, one)` - l += ones x P^T on the packed e4m3 P; PHalf has no add"),
    "fast": ("byte", "rounded", "the same j4; P is the byte of PHalf<ABL, 1>::step (v_cvt_pk_u8_f32 of 8 (s - m_run + 5) + 56, saturating at 0)"),
}
# A key exponentiated against a running maximum `d` octaves above it reaches the numerator iff d < KEPT_BELOW: exp2 forms - e4m3(2^(5 - d))
# is 2^-9 for 14 <= d < 15 and 0 from the tie d = 15 on; fast form - the byte rne(96 - 8 d) is 0 from d = 12 on (2^-7 would be byte 4:
# the byte is exponent-field arithmetic, and under 2^-6 e4m3's exponent field is spent - bytes 1 .. 7 are the linear subnormals).
KEPT_BELOW = {"exp2": 15.0, "byte": 12.0}


def kernel_of(form, tiles):
    """The kernel am_attention_fp8 runs on the main grid of a call that walks `tiles` key tiles (its dispatch: the product and 4 x 64
    kernels need 8 tiles; below that every form but the refused 100 runs the 8-wave kernel, fp8_fast in the exact-exp2 form)."""
    assert form in FORMS
    if form == 200 or tiles < 8:
        assert form != 100 or tiles >= 8, "the dispatch refuses the 4 x 64 form on a short stream"
        return "wave8"
    return {0: "product", 100: "x64", 400: "fast"}[form]


def e4m3(x):
    """fp64 -> the nearest e4m3 value (ties to even, subnormals of 2^-9), by torch's CPU conversion."""
    return x.float().to(torch.float8_e4m3fn).double()


def fast_byte(d):
    """The fast form's probability of a key d octaves under m_run: the byte rne(8 (5 - d) + 56), saturating at 0, read as e4m3."""
    b = torch.round(8.0 * (P_SHIFT - d) + 56.0).clamp(0, 255).to(torch.uint8)
    return b.view(torch.float8_e4m3fn).double()


Case = namedtuple("Case", "q k v v1 s dom chunk_tiles shape G where profile")


def case(nseq, H, sq, skc, P, G, where, profile):
    """fp32 operands on the CPU (q (nseq, H, sq, 128), k / v / v1 (nseq, H, skc * P, 128)), the fp64 score of every key, the dominant
    key's index, and per chunk the list of its tiles' key indices.  `last` with skc % 64 != 0 puts the dominant key in a partial tile
    beside the masked pad keys."""
    assert where in WHERE and profile in PROFILES
    n = skc * P
    tiles_c = -(-skc // TILE)
    j = torch.arange(skc).repeat(P)                                        # index of a key inside its chunk
    gt = torch.arange(P).repeat_interleave(skc) * tiles_c + j // TILE      # global tile of a key
    dom = {"first": 0, "last": n - 1, "middle": (2 * skc + skc // 2) if P >= 3 else n // 2}[where]
    s = torch.zeros(n, dtype=torch.float64) if profile == "pow2" else -(j % 8).double() / 8.0
    s[dom] = float(G)
    q = torch.zeros((nseq, H, sq, X.D))
    q[..., 0] = 1.0
    k = torch.zeros((nseq, H, n, X.D))
    k[..., 0] = s.float()
    v = torch.zeros((n, X.D))
    v[torch.arange(n), gt % X.D] = 1.0
    v[dom] = 1.0 + (torch.arange(X.D) % 8).float() / 8.0
    v = v.expand(nseq, H, n, X.D).contiguous()
    chunk_tiles = [[torch.arange(c * skc + t * TILE, c * skc + min(skc, (t + 1) * TILE)) for t in range(tiles_c)] for c in range(P)]
    cs = Case(q, k, v, torch.ones_like(v), s, dom, chunk_tiles, (nseq, H, sq, skc, P), G, where, profile)
    conditions(cs)
    return cs


def tie_distance(p):
    """Distance of every value of p (fp64, > 0) from the nearest e4m3 rounding tie, in units of e4m3's spacing at that value."""
    e = torch.floor(torch.log2(p)).clamp_min(-6.0)                         # under 2^-6 the spacing stays 2^-9
    steps = p / torch.exp2(e - 3.0)
    return (steps - torch.floor(steps) - 0.5).abs()


def conditions(cs):
    """What a case promises, on the operands alone: they survive e4m3 (and bf16) bit for bit; Q' = Q; the fp64 score of every key is
    cs.s, the dominant key stands G >= 8 above the tail's best (the deferred re-base cannot lag); and every probability the exp2 forms
    can form of a tail key - against the tail's own maximum (before the dominant key is seen) or against G (after) - is either exactly
    2^integer or at least 2^-8 of a spacing away from an e4m3 tie, far above v_exp_f32's error.  Returns the smallest such distance."""
    X.round_trips(cs.q, cs.k, cs.v, cs.v1)
    c = torch.tensor(X.SCALE, dtype=torch.float32) * torch.tensor(X.LOG2E_F32, dtype=torch.float32)
    assert float(c) == 1.0
    s = (cs.q[0, 0, 0].double() @ cs.k[0, 0].double().T)
    assert torch.equal(s, cs.s) and bool((cs.q == cs.q[0, 0, 0]).all()) and bool((cs.k == cs.k[0, 0]).all())
    tail = torch.cat([cs.s[:cs.dom], cs.s[cs.dom + 1:]])
    assert float(tail.max()) == 0.0 and float(tail.min()) > -1.0 and cs.G - float(tail.max()) >= 8
    for chunk in cs.chunk_tiles:
        for idx in chunk:
            assert float(cs.s[idx].max()) >= 0.0, "a tile whose maximum is not the tail's (or the dominant key)"
    frac = tail[tail != tail.round()]
    worst = 0.5
    if frac.numel():
        worst = min(float(tie_distance(torch.exp2(P_SHIFT + frac)).min()), float(tie_distance(torch.exp2(P_SHIFT - cs.G + frac)).min()))
        assert worst >= 2.0 ** -8, f"a tail probability {worst:.2e} of a spacing from an e4m3 tie"
    return worst


def softmax_fp64(cs, v):
    """The plain fp64 base-2 softmax attention of one row -> (128,)."""
    w = torch.exp2(cs.s - cs.s.max())
    return (w @ v[0, 0].double()) / w.sum()


class Walk:
    """Online softmax of one query row as a kernel runs it, in fp64: O, l carry the factor 2^5; `dropped` collects the keys whose
    probability was packed as 0.  The kernels decide a re-base per wave (a ballot over its 32 rows) and then shift each row by its own
    excess; every row of a case is alike - and a pad row, whose Q is 0, never exceeds - so the row's own condition is the wave's.
    With the tail at 0 and G >= 8 > 2^3 the deferred maximum never lags: m_run is the maximum of what has been seen."""

    def __init__(self, cs, v, kernel, rounded=None):
        self.s, self.v = cs.s, v[0, 0].double()
        self.prob, rowsum, _ = KERNELS[kernel]
        self.rounded = (rowsum == "rounded") if rounded is None else rounded
        self.m, self.l, self.O, self.dropped = None, 0.0, torch.zeros(X.D, dtype=torch.float64), []

    def tile(self, idx):
        st = self.s[idx]
        mx = float(st.max())
        if self.m is None:                                                 # the first tile sets m_run
            self.m = mx
        elif mx - self.m > DEFER:                                          # deferred re-base: what was accumulated is rescaled in fp32
            a = 2.0 ** (self.m - mx)
            self.O, self.l, self.m = self.O * a, self.l * a, mx
        p = torch.exp2(st - self.m + P_SHIFT)
        p8 = e4m3(p) if self.prob == "exp2" else fast_byte(self.m - st)
        self.l += float((p8 if self.rounded else p).sum())
        self.O = self.O + p8 @ self.v[idx]
        self.dropped.append(idx[p8 == 0])
        return self

    def tiles(self, tiles):
        for idx in tiles:
            self.tile(idx)
        return self


def _stream(cs, chunks):
    return [idx for c in chunks for idx in cs.chunk_tiles[c]]


def tail_rows(sq):
    """Rows of the short last query block that runs in a launch of its own on the 8-wave kernel (am_attn_plan_qblocks: at least nine
    256-row blocks and at most 128 rows in the last), else 0."""
    nblk = -(-sq // 256)
    rest = sq - (nblk - 1) * 256
    return rest if nblk >= 9 and rest <= 128 else 0


def emulate(cs, v, form, rank=None, swap_rowsum=False, reverse=False):
    """Expected output of ops.attention_fp8(..., ablate=form), fp64 (sq, 128), and the share of the fp64 softmax mass whose keys the
    main grid packs as 0.  rank = None: one pass over the chunks in order.  rank = r: rank r's two-pass view - chunk r alone (state
    saved), then resumed over chunks r + 1 .. r - 1 in ring order.  The short last block (tail_rows) is the 8-wave kernel over the
    natural order, cut SPLIT_Z ways into independent key ranges merged in fp32 when the stream has 4 SPLIT_Z tiles.
    swap_rowsum / reverse: the two WRONG emulators of the CPU test - the other row-sum convention; the tiles walked backwards, which
    swaps the tiles seen before the dominant key with those seen after."""
    nseq, H, sq, skc, P = cs.shape
    tiles_c = len(cs.chunk_tiles[0])

    def walk(kernel):
        return Walk(cs, v, kernel, None if not swap_rowsum else KERNELS[kernel][1] != "rounded")

    if rank is None:
        stream = _stream(cs, range(P))
        w = walk(kernel_of(form, len(stream))).tiles(stream[::-1] if reverse else stream)
    else:
        w = walk(kernel_of(form, tiles_c)).tiles(_stream(cs, [rank]))
        resumed = _stream(cs, [(rank + 1 + i) % P for i in range(P - 1)])
        w2 = walk(kernel_of(form, len(resumed)))
        w2.m, w2.l, w2.O, w2.dropped = w.m, w.l, w.O, w.dropped          # (O, m, l) through the state buffer
        w = w2.tiles(resumed)
    out = (w.O / w.l).expand(sq, X.D).clone()
    true = torch.exp2(cs.s - cs.s.max())
    lost = float(true[torch.cat(w.dropped)].sum() / true.sum())
    rest = tail_rows(sq)
    if rest:
        stream = _stream(cs, range(P))
        T = len(stream)
        if T >= 4 * SPLIT_Z:
            parts = [Walk(cs, v, "wave8").tiles(stream[z * T // SPLIT_Z:(z + 1) * T // SPLIT_Z]) for z in range(SPLIT_Z)]
        else:
            parts = [Walk(cs, v, "wave8").tiles(stream)]
        m = max(p.m for p in parts)                                        # attn_combine_kernel
        O = sum(p.O * 2.0 ** (p.m - m) for p in parts)
        l = sum(p.l * 2.0 ** (p.m - m) for p in parts)
        out[sq - rest:] = O / l
    return out, lost


def full(rows, cs):
    """(sq, 128) -> the layout of the kernels' output, (nseq * sq, H * 128): every sequence and head alike."""
    nseq, H = cs.shape[:2]
    return rows.repeat(nseq, H)


def in_range(cs, form, tiles):
    """The emulator of this form is the plain fp64 softmax: every tail key lies inside the form's range whatever the order."""
    prob = KERNELS[kernel_of(form, tiles)][0]
    # a non-integer score is rounded to e4m3's three mantissa bits wherever it is seen: only powers of two come through unchanged
    return cs.profile == "pow2" and cs.G < KEPT_BELOW[prob]


# The cases of the GPU test: (nseq, H, sq, skc, P) x G.  3300 keys in 54 tiles with a partial last tile per chunk (product kernel);
# the short stream, where the dispatch falls to the 8-wave kernel; the two-pass / split-tail shape of test_attention_exact_gpu.py.
SHAPE_LONG, SHAPE_SHORT, SHAPE_TWO_PASS = (1, 1, 300, 1100, 3), (1, 1, 300, 257, 1), (2, 2, 2320, 1100, 4)
GS = (8, 11, 12, 14, 15, 16)             # inside every range; 12, 14: past the fast form's; 15: the tie; 16: past all


def forms_of(shape):
    return tuple(f for f in FORMS if f != 100 or -(-shape[3] // TILE) * shape[4] >= 8)

