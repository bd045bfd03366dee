"""The fp64 emulator of tests/_fp8_range.py held against what it claims to be, without a GPU: inside every form's range it IS the plain
fp64 softmax; at the edges it drops exactly the keys its table names; its cases keep the promises the GPU test relies on; and an
emulator with one convention wrong stands further from the right one than the GPU comparison allows - the comparison has teeth."""
import pytest
import torch

import _attention_exact as X
import _fp8_range as R

CASES = [(shape, G) for shape in (R.SHAPE_LONG, R.SHAPE_SHORT, R.SHAPE_TWO_PASS) for G in R.GS]


def _views(shape):
    """(rank, tiles the form's dispatch sees): the one-pass view of every shape, and every rank's two-pass view of the chunked one."""
    nseq, H, sq, skc, P = shape
    tiles_c = -(-skc // R.TILE)
    return [(None, tiles_c * P)] + ([(r, tiles_c) for r in range(P)] if shape == R.SHAPE_TWO_PASS else [])


def test_e4m3_rounding_at_the_subnormal_ties():
    """torch's CPU conversion, which the emulator rounds with: 2^-9 is the smallest subnormal; the ties go to the even neighbour."""
    u = 2.0 ** -10
    x = torch.tensor([2 * u, u, 1.5 * u, 3 * u, 0.5 * u, 5 * u, 448.0, 2.0 ** -6, 2.0 ** -6 - u], dtype=torch.float64)
    want = torch.tensor([2 * u, 0.0, 2 * u, 4 * u, 0.0, 4 * u, 448.0, 2.0 ** -6, 2.0 ** -6], dtype=torch.float64)
    assert torch.equal(R.e4m3(x), want)
    assert torch.equal(R.e4m3(-x), -want)
    # the fast form's byte: exact at whole octaves down to 11 (byte 8 = 2^-6), linear subnormals below, 0 from 12 octaves on
    d = torch.tensor([0.0, -3.0, 11.0, 11.125, 11.875, 12.0, 14.0, 11.9375, 11.8125], dtype=torch.float64)
    want = torch.tensor([32.0, 256.0, 2.0 ** -6, 7 * 2 * u, 2 * u, 0.0, 0.0, 0.0, 2.0 * 2 * u], dtype=torch.float64)
    assert torch.equal(R.fast_byte(d), want)      # 11.9375 -> byte 0.5 -> 0 and 11.8125 -> byte 1.5 -> 2: ties to even


@pytest.mark.parametrize("shape,G", CASES)
def test_cases_keep_their_promises(shape, G):
    """The quantiser identity and the tie-distance condition for every case of the GPU table (R.case asserts them; here the smallest
    distance is shown - the issue's own measurement: 0.0137 spacings, 2^0.25 x 8 = 9.514)."""
    worst = 0.5
    for where in R.WHERE:
        for profile in R.PROFILES:
            cs = R.case(*shape, G, where, profile)
            worst = min(worst, R.conditions(cs))
            nseq, H, sq, skc, P = shape
            assert cs.k.shape == (nseq, H, skc * P, X.D) and float(cs.s[cs.dom]) == G and int((cs.s > 0).sum()) == 1
            if where == "last" and skc % R.TILE:
                assert cs.chunk_tiles[-1][-1].numel() == skc % R.TILE and int(cs.chunk_tiles[-1][-1][-1]) == cs.dom
    print(f"{shape} G={G}: closest tail probability {worst:.4f} of an e4m3 spacing from a tie")
    assert worst >= 2.0 ** -8


@pytest.mark.parametrize("shape,G", CASES)
def test_emulator_is_the_fp64_softmax_inside_the_range(shape, G):
    """pow2 profile, G under the form's limit: bit-equal to the plain fp64 softmax in every view (powers of two: every sum is exact),
    nothing dropped, and V = 1 gives exactly 1."""
    seen = 0
    for where in R.WHERE:
        cs = R.case(*shape, G, where, "pow2")
        ref = R.softmax_fp64(cs, cs.v)
        for form in R.forms_of(shape):
            for rank, tiles in _views(shape):
                if not R.in_range(cs, form, tiles):
                    continue
                out, lost = R.emulate(cs, cs.v, form, rank)
                one, _ = R.emulate(cs, cs.v1, form, rank)
                assert lost == 0.0 and torch.equal(out, ref.expand_as(out)) and bool((one == 1.0).all()), (where, form, rank)
                seen += 1
    assert seen > 0 or G >= 15


def _after(cs, stream):
    """Tail keys of `stream` (a list of tiles in walk order) that are exponentiated against the dominant key's maximum: those of its
    own tile and of every later one."""
    at = next(i for i, idx in enumerate(stream) if bool((idx == cs.dom).any()))
    keys = torch.cat(stream[at:])
    return keys[keys != cs.dom]


@pytest.mark.parametrize("G", R.GS)
@pytest.mark.parametrize("profile", R.PROFILES)
def test_emulator_drops_exactly_the_keys_the_table_names(G, profile):
    """One pass over 3300 keys: a key seen before the dominant one is never dropped; one seen with or after it, d = G + f octaves under
    m_run, is dropped iff d >= KEPT_BELOW of the form's probability (15: the 2^-10 tie goes to 0; 12 for the fast form's byte).  The
    reported share is those keys' share of the fp64 softmax mass."""
    for where in R.WHERE:
        cs = R.case(*R.SHAPE_LONG, G, where, profile)
        stream = R._stream(cs, range(3))
        after = _after(cs, stream)
        true = torch.exp2(cs.s - G)
        for form in R.FORMS:
            kernel = R.kernel_of(form, len(stream))
            w = R.Walk(cs, cs.v, kernel).tiles(stream)
            dropped = torch.cat(w.dropped).sort().values
            want = after[(G - cs.s[after]) >= R.KEPT_BELOW[R.KERNELS[kernel][0]]].sort().values
            assert torch.equal(dropped, want), (where, form)
            _, lost = R.emulate(cs, cs.v, form)
            assert lost == float(true[want].sum() / true.sum())
    if profile == "pow2":          # the issue's figures: 3299 tail keys behind the dominant one
        cs = R.case(*R.SHAPE_LONG, G, "first", "pow2")
        share = 3299 * 2.0 ** -G / (1 + 3299 * 2.0 ** -G)
        for form in R.FORMS:
            past = G >= R.KEPT_BELOW[R.KERNELS[R.kernel_of(form, 54)][0]]
            assert abs(R.emulate(cs, cs.v, form)[1] - (share if past else 0.0)) < 1e-12
        assert G != 15 or abs(share - 0.0915) < 1e-4
        assert G != 12 or abs(share - 0.446) < 1e-3


def test_row_sum_conventions_past_the_range():
    """G = 16, dominant key first: every tail key but none of the mass of the dominant one is dropped.  A kernel that sums the ROUNDED
    probabilities renormalises over the survivors - the dominant key alone: the output is its V, and V = 1 gives 1; one that sums the
    UNROUNDED ones scales the whole output down by the lost share."""
    cs = R.case(*R.SHAPE_LONG, 16, "first", "pow2")
    vd = cs.v[0, 0, cs.dom].double()
    for form in R.FORMS:
        out, lost = R.emulate(cs, cs.v, form)
        one, _ = R.emulate(cs, cs.v1, form)
        if R.KERNELS[R.kernel_of(form, 54)][1] == "rounded":
            assert torch.equal(out[0], vd) and bool((one == 1.0).all())
        else:
            assert torch.allclose(out[0], vd * (1.0 - lost), rtol=1e-15, atol=0) and torch.allclose(one, torch.full_like(one, 1.0 - lost), rtol=1e-15)


def _miss(a, b, n_keys):
    """max |a - b| over the GPU comparison's bound on b (X.bound with a bf16 output): above 1, a kernel that did `a` fails against `b`."""
    return float(((a - b).abs() / X.bound(b, n_keys, "bf16")).max())


@pytest.mark.parametrize("G", [12, 15, 16])
def test_a_wrong_emulator_is_rejected(G):
    """The two mistakes the GPU comparison exists to catch, made on purpose: the row-sum conventions swapped between the kernels, and
    the tiles seen before / after the dominant key swapped (the stream walked backwards).  Past a form's range each must miss the
    right emulator by more than the comparison's bound - at 3300 keys the lost share is 9.1 % at G = 15 (44.6 % at G = 12 in the fast
    form) against an output rounding of 2^-8 - on V or on its V = 1 twin."""
    n = 3300
    for form in R.FORMS:
        prob = R.KERNELS[R.kernel_of(form, 54)][0]
        if G < R.KEPT_BELOW[prob]:
            continue
        for where in ("first", "middle"):          # `last`: nothing but its own tile is seen after the dominant key
            cs = R.case(*R.SHAPE_LONG, G, where, "pow2")
            good = {v: R.emulate(cs, getattr(cs, v), form)[0] for v in ("v", "v1")}
            swapped = max(_miss(R.emulate(cs, getattr(cs, v), form, swap_rowsum=True)[0], good[v], n) for v in ("v", "v1"))
            assert swapped > 1.0, (form, where, swapped)
            if where == "first":
                backwards = max(_miss(R.emulate(cs, getattr(cs, v), form, reverse=True)[0], good[v], n) for v in ("v", "v1"))
                assert backwards > 1.0, (form, backwards)
                print(f"G={G} form {form}: swapped row sums miss by {swapped:.1f} x bound, swapped order by {backwards:.1f} x bound")


def test_two_pass_views_differ_by_what_each_rank_sees_first():
    """G = 15, dominant key in chunk 2 of 4: rank 2 meets it in its own chunk and exponentiates the three other chunks against it
    (they are dropped); rank 3 has walked its own chunk before - kept - and so on round the ring; the short last block is the same for
    every rank (natural order, 16 independent key ranges: only the range that holds the dominant key can drop anything)."""
    cs = R.case(*R.SHAPE_TWO_PASS, 15, "middle", "pow2")
    lost = [R.emulate(cs, cs.v, 0, r)[1] for r in range(4)]
    true = torch.exp2(cs.s - 15.0)
    per_chunk = float(true[:1100].sum() / true.sum())
    half = float(true[2 * 1100 + 550 - 550 % 64:3 * 1100].sum() - 1.0) / float(true.sum())       # its own tile on, without itself
    want = [half + per_chunk * n for n in (1, 2, 3, 0)]          # rank r resumes over chunks r+1 ..: those after chunk 2 in ITS order
    assert all(abs(a - b) < 1e-12 for a, b in zip(lost, want)), (lost, want)
    tails = [R.emulate(cs, cs.v, 0, r)[0][-1] for r in range(4)]
    assert all(torch.equal(t, tails[0]) for t in tails) and not torch.equal(tails[0], R.emulate(cs, cs.v, 0, 2)[0][0])
