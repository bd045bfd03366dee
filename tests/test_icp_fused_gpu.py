"""am_icp_step on the device against its contract restated in numpy (tests/_icp_ref.py): the 26 sums within the fp64 reordering bound,
the tie rule on exact lattice data, the chain rule and Adam bit for bit from the device's own sums, the best-so-far record, the fused
gradient_icp against the autograd one, determinism, non-finite inputs, guard bands and refused arguments."""
import numpy as np
import pytest
import torch

import _icp_ref as REF
from _guard import Arena, Padded64
from actionmesh_amd import _lib, actionbench as AB, ops

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1, 1), (3, 37, 5), (24, 255, 257), (24, 700, 1100)]
F32_FIELDS = ("params", "adam_m", "adam_v", "best", "out_loss", "out_rot")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def canonical(B):
    R = AB.canonical_rotation_matrices().numpy().reshape(24, 9)
    return R.copy() if B == 24 else R[[9, 17, 5][:B]].copy()


def make_case(B, P, Q, seed=0):
    """random Gaussian clouds and a perturbed state with a non-trivial Adam history"""
    rng = np.random.default_rng(100 * seed + B + P + Q)
    pred = (rng.standard_normal((P, 3)) * [1.0, 0.6, 0.3]).astype(np.float32)
    gt = (rng.standard_normal((Q, 3)) * [0.9, 0.7, 0.4] + [0.1, -0.05, 0.02]).astype(np.float32)
    st = REF.State(B)
    st.params = (st.params + 0.1 * rng.standard_normal((B, 12))).astype(np.float32)
    st.adam_m = (1e-2 * rng.standard_normal((B, 12))).astype(np.float32)
    st.adam_v = (1e-4 * rng.standard_normal((B, 12)) ** 2).astype(np.float32)
    return pred, gt, canonical(B), st


_CASES = {}


def case_of(shape):
    """the case of a shape with the restatement's sums, computed once and shared (never modified)"""
    if shape not in _CASES:
        pred, gt, rot, st = make_case(*shape)
        _CASES[shape] = (pred, gt, rot, st, REF.sums_of(pred, gt, st.params, rot))
    return _CASES[shape]


def load(st, dev):
    """a REF.State into an ops.IcpState"""
    d = ops.IcpState(len(st.params), dev)
    for name in ("params", "adam_m", "adam_v", "best"):
        getattr(d, name).copy_(torch.from_numpy(getattr(st, name)))
    return d


def to_dev(dev, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def within_one_ulp32(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return bool((np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.maximum(np.abs(a), np.abs(b)))).all())


def sums_bound(mags, counts):
    """the fp64 reordering bound of a sum of N terms: N 2^-52 sum|terms|"""
    return counts[:, :, None] * 2.0 ** -52 * mags


# ------------------------------------------------------------------------------------------------------------------ 1. sums
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sums_loss_and_rotation_against_the_restatement(shape, dev):
    """fewer points than a wave, a partial workgroup, a partial 512-point tile, more than one tile, more than one workgroup, P != Q both
    ways"""
    B, P, Q = shape
    pred, gt, rot, st, (sums, mags, counts, flag) = case_of(shape)
    assert flag == 0
    d = load(st, dev)
    tp, tg, tr = to_dev(dev, pred, gt, rot)
    ops.icp_step(d, tp, tg, tr, t=3, update=False, return_sums=True)
    got = d.out_sums.cpu().numpy()
    err, bound = np.abs(got - sums), sums_bound(mags, counts)
    print(f"{shape}: worst |diff| / bound {np.max(err / np.maximum(bound, 1e-300)):.3e}, max |diff| {err.max():.3e}")
    assert (err <= bound).all()
    assert int(d.out_flag.cpu()) == 0
    ref = st.copy()
    REF.step(ref, pred, gt, rot, t=3, update=False, sums=sums)
    assert same_bits(d.out_rot, ref.out_rot)                               # no sum feeds R
    assert within_one_ulp32(d.out_loss.cpu().numpy(), ref.out_loss)        # the sums feed the loss
    own = st.copy()
    REF.step(own, pred, gt, rot, t=3, update=False, sums=got)
    assert same_bits(d.out_loss, own.out_loss) and same_bits(d.out_grad, own.out_grad)
    for name in ("params", "adam_m", "adam_v", "best"):                    # update = 0 leaves the state untouched
        assert same_bits(getattr(d, name), getattr(st, name)), name


# ------------------------------------------------------------------------------------------------------------------ 2. tie rule
def test_ties_go_to_the_lowest_index_on_exact_data(dev):
    """integer lattice coordinates, the identity state and R_init rounded to the signed permutations they stand for: every operation
    is exact, so the sums are the restatement's whatever the order.  Every pred point p has the six gt points p +- 2 e_k at the same
    distance (direction 0), and gt points midway between two pred points 8 apart (direction 1): residuals of opposite sign, so the
    wrong winner changes the sums."""
    rng = np.random.default_rng(5)
    cells = rng.permutation(17 ** 3)[:250]
    base = (np.stack((cells % 17, cells // 17 % 17, cells // 289), -1) - 8) * 16          # distinct, 16 apart
    pred = np.concatenate((base, base[:60] + [8, 0, 0])).astype(np.float32)
    pred = pred[rng.permutation(len(pred))]
    six = np.concatenate([np.eye(3) * 2, np.eye(3) * -2])
    gt = np.concatenate(((pred[:, None, :] + six[None]).reshape(-1, 3), base[:60] + [4, 0, 0])).astype(np.float32)
    gt = gt[rng.permutation(len(gt))]
    rot = np.round(AB.canonical_rotation_matrices().numpy()).astype(np.float32).reshape(24, 9)
    assert (np.abs(rot).reshape(24, 3, 3).sum(1) == 1).all() and (np.abs(rot).reshape(24, 3, 3).sum(2) == 1).all()
    st = REF.State(24)
    # candidate 0 is the identity: the ties are there, in both directions
    d0 = ((pred[:, None, :] - gt[None]) ** 2).sum(-1)
    assert ((d0 == d0.min(1, keepdims=True)).sum(1) == 6).all() and ((d0 == d0.min(0, keepdims=True)).sum(0) == 2).sum() == 60
    sums, mags, counts, flag = REF.sums_of(pred, gt, st.params, rot)
    last = REF.sums_of(pred[::-1], gt[::-1], st.params, rot)[0]              # the other winners: the sums do depend on the rule
    assert flag == 0 and not np.array_equal(last[0], sums[0])
    d = load(st, dev)
    ops.icp_step(d, *to_dev(dev, pred, gt, rot), t=1, update=False, return_sums=True)
    got = d.out_sums.cpu().numpy()
    assert np.array_equal(got, sums)           # exact values (array_equal reads -0 and +0 as the same exact sum)
    assert len(pred) > 64 and len(gt) > 2 * 512


# ------------------------------------------------------------------------------------------------------------------ 3. update
@pytest.fixture(scope="module")
def trajectory():
    """the restatement's states after 0, 1 and 7 iterations from the reference's start"""
    B, P, Q = 24, 255, 257
    pred, gt, rot, _ = make_case(B, P, Q, seed=3)
    st, states = REF.State(B), {}
    for t in range(1, 9):
        if t - 1 in (0, 1, 7):
            states[t - 1] = st.copy()
        REF.step(st, pred, gt, rot, t=t)
    return pred, gt, rot, states


@pytest.mark.parametrize("done", [0, 1, 7])
def test_chain_rule_and_adam_bit_for_bit_from_the_devices_sums(done, trajectory, dev):
    pred, gt, rot, states = trajectory
    st = states[done]
    d = load(st, dev)
    ops.icp_step(d, *to_dev(dev, pred, gt, rot), t=done + 1, return_sums=True)
    own = st.copy()
    REF.step(own, pred, gt, rot, t=done + 1, sums=d.out_sums.cpu().numpy())
    for name in ("params", "adam_m", "adam_v", "out_grad", "out_loss", "out_rot", "best"):
        assert same_bits(getattr(d, name), getattr(own, name)), name
    sums, mags, counts, _ = REF.sums_of(pred, gt, st.params, rot)
    ref = st.copy()
    REF.step(ref, pred, gt, rot, t=done + 1, sums=sums)
    for name in ("params", "adam_m", "adam_v", "out_loss"):
        assert within_one_ulp32(getattr(d, name).cpu().numpy(), getattr(ref, name)), name
    assert np.abs(d.params.cpu().numpy() - st.params).max() > 1e-3            # a step was taken
    # the fp64 gradient from the restatement's own sums: the reordering bound of the sums through the (linear) chain rule
    bound = np.stack([np.abs(REF.jacobian(st.params[b], rot[b], len(pred), len(gt), 24)[1:]) @ sums_bound(mags, counts)[b].reshape(26)
                      for b in range(24)])
    assert (np.abs(d.out_grad.cpu().numpy() - ref.out_grad) <= bound).all()


# ------------------------------------------------------------------------------------------------------------------ 4. best so far
def test_best_so_far_keeps_the_rotation_before_and_the_rest_after_the_update(dev):
    pred, gt, rot, _ = make_case(24, 255, 257, seed=4)
    tp, tg, tr = to_dev(dev, pred, gt, rot)
    d = ops.IcpState(24, dev)
    best_loss, changed = np.float32(np.inf), 0
    for t in range(1, 6):
        before = d.best.cpu().numpy().copy()
        ops.icp_step(d, tp, tg, tr, t=t)
        loss, best = d.out_loss.cpu().numpy(), d.best.cpu().numpy()
        c = int(np.argmin(loss))                                              # first minimum
        if loss[c] < best_loss:
            best_loss, changed = loss[c], changed + 1
            want = np.concatenate((d.out_rot.cpu().numpy()[c], d.params.cpu().numpy()[c, 0:3], d.params.cpu().numpy()[c, 9:12], [loss[c]]))
            assert same_bits(best, want.astype(np.float32)), t                # R of this iteration, T and s after its update
        else:
            assert same_bits(best, before), t
    assert changed >= 2
    # an iteration whose minimum is not strictly lower: the stored loss set to exactly the minimum to come, markers around it
    ops.icp_step(d, tp, tg, tr, t=6, update=False)
    coming = d.out_loss.cpu().numpy().min()
    keep = {name: getattr(d, name).clone() for name in ("params", "adam_m", "adam_v")}
    marker = torch.arange(16, dtype=torch.float32, device=dev) + 100
    marker[15] = float(coming)
    d.best.copy_(marker)
    ops.icp_step(d, tp, tg, tr, t=6)
    assert same_bits(d.best, marker) and not same_bits(d.params, keep["params"])
    for name, val in keep.items():
        getattr(d, name).copy_(val)
    marker[15] = float(np.nextafter(coming, np.float32(np.inf)))
    d.best.copy_(marker)
    ops.icp_step(d, tp, tg, tr, t=6)
    assert float(d.best[15]) == float(coming) and not same_bits(d.best[:15], marker[:15])


# ------------------------------------------------------------------------------------------------------------------ 5. the existing path
def test_fused_gradient_icp_meets_the_autograd_paths_bars(dev):
    """the data and the bars of test_actionbench.py::test_gradient_icp_recovers_a_known_similarity; the comparison run is the autograd
    path on the same device"""
    g = torch.Generator().manual_seed(4)
    pred = torch.randn((500, 3), generator=g) * torch.tensor([1.0, 0.6, 0.3]) + torch.tensor([0.3, 0.0, 0.0]) * torch.randn((500, 1), generator=g).abs()
    R_true = AB.canonical_rotation_matrices()[9] @ AB.euler_angles_to_matrix(torch.tensor([0.21, -0.1, 0.05]))
    gt = (torch.tensor([1.1, 0.95, 1.05]) * pred) @ R_true + torch.tensor([0.05, -0.02, 0.03])
    gt = gt[torch.randperm(500, generator=g)]
    icp = AB.gradient_icp(pc_pred=pred.to(dev), pc_gt=gt.to(dev), lr=0.01, n_iter=120, step="fused")
    assert isinstance(icp, AB.ScaleRotateTranslate) and len(icp) == 1 and icp.R.device.type == "cuda"
    before = AB.compute_chamfer_score(pred, gt)
    after = AB.compute_chamfer_score(icp.transform_points(pred.to(dev)), gt)
    auto = AB.gradient_icp(pc_pred=pred.to(dev), pc_gt=gt.to(dev), lr=0.01, n_iter=120, step="autograd")
    print(f"before {before:.4e} after {after:.4e} fused loss {icp.loss:.6e} autograd loss {auto.loss:.6e}")
    assert after < 0.1 * before and icp.loss < 2e-3, (before, after, icp.loss)
    assert abs(icp.loss - auto.loss) <= 0.25 * max(auto.loss, 1e-4), (icp.loss, auto.loss)
    cd3, cd4, cdm = AB.compute_chamfer_3d_4d(gt[None].repeat(2, 1, 1), pred[None].repeat(2, 1, 1), device=dev, is_4D=True,
                                             pred_pc_4D=pred[None].repeat(2, 1, 1), n_pts_icp=300, n_iter=60, icp="fused")
    assert all(np.isfinite(v) for v in (cd3, cd4, cdm)) and 0 <= cd3 < before and 0 <= cd4 < before and cdm >= 0, (cd3, cd4, cdm, before)


# ------------------------------------------------------------------------------------------------------------------ 6. determinism
def test_two_fused_runs_give_the_same_bits(dev):
    pred, gt, rot, _ = make_case(24, 700, 1100, seed=6)
    tp, tg, tr = to_dev(dev, pred, gt, rot)
    runs = []
    for _ in range(2):
        d = ops.IcpState(24, dev)
        for t in range(1, 31):
            ops.icp_step(d, tp, tg, tr, t=t)
        runs.append(d)
    for name in ("best", "params", "out_loss", "adam_m", "adam_v"):
        assert same_bits(getattr(runs[0], name), getattr(runs[1], name)), name
    assert float(runs[0].best[15]) < float("inf")


# ------------------------------------------------------------------------------------------------------------------ 7. non-finite input
@pytest.mark.parametrize("which", ["pred", "gt"])
def test_a_nan_coordinate_is_flagged_and_never_indexed(which, dev):
    """a NaN point is nobody's neighbour and has none.  As a query it contributes no term and sets the flag; as a point it changes
    nothing: the direction in which it is a point has the sums, bit for bit, of the run in which that point lies far away instead.
    The inputs sit in poisoned arenas: a gather at index -1 would read a NaN guard and show in the sums."""
    B, P, Q = 3, 300, 280
    pred, gt, rot, st = make_case(B, P, Q, seed=7)
    bad, far = {"pred": pred.copy(), "gt": gt.copy()}, {"pred": pred.copy(), "gt": gt.copy()}
    bad[which][131, 1] = np.nan
    far[which][131] = 1e6
    sums, mags, counts, flag = REF.sums_of(bad["pred"], bad["gt"], st.params, rot)
    query_dir = 0 if which == "pred" else 1
    assert flag == REF.NO_NEIGHBOUR and (counts[:, query_dir] == (P if which == "pred" else Q) - 1).all() and (counts[:, 1 - query_dir] == (Q if which == "pred" else P)).all()
    out = {}
    for name, data in (("bad", bad), ("far", far)):
        d = load(st, dev)
        tp, tg, tr = (Arena.flat_of(t).view for t in to_dev(dev, data["pred"], data["gt"], rot))
        ops.icp_step(d, tp, tg, tr, t=3, update=False, return_sums=True)
        out[name] = (d.out_sums.cpu().numpy(), int(d.out_flag.cpu()), d.out_loss.cpu().numpy())
    got, got_flag, loss = out["bad"]
    assert got_flag == _lib.ICP_NO_NEIGHBOUR and out["far"][1] == 0
    assert np.isfinite(got).all() and np.isfinite(loss).all()
    assert (np.abs(got - sums) <= sums_bound(mags, counts)).all()
    assert same_bits(got[:, 1 - query_dir], out["far"][0][:, 1 - query_dir])
    tp, tg = to_dev(dev, bad["pred"], bad["gt"])
    with pytest.raises(ValueError, match="no finite distance"):
        AB.gradient_icp(pc_pred=tp, pc_gt=tg, n_iter=2, step="fused")


# ------------------------------------------------------------------------------------------------------------------ 8. guard bands
@pytest.mark.parametrize("shape", [(3, 37, 5), (24, 700, 1100)], ids=lambda s: "x".join(map(str, s)))
def test_guard_bands_around_every_buffer(shape, dev):
    B, P, Q = shape
    pred, gt, rot, st, _ = case_of(shape)
    tp, tg, tr = to_dev(dev, pred, gt, rot)
    plain = load(st, dev)
    ops.icp_step(plain, tp, tg, tr, t=3, return_sums=True)
    d = load(st, dev)
    arenas = {}
    for name in F32_FIELDS:
        arenas[name] = Arena.flat(getattr(d, name).shape, torch.float32, dev)
        arenas[name].view.copy_(getattr(d, name))
        setattr(d, name, arenas[name].view)
    arenas["out_flag"] = Arena.flat((1,), torch.int32, dev)
    arenas["out_flag"].view.zero_()
    d.out_flag = arenas["out_flag"].view
    p64 = {"out_sums": Padded64((B, 2, 13), dev, 12345.0), "out_grad": Padded64((B, 12), dev, 12345.0)}
    d.out_sums, d.out_grad = p64["out_sums"].view, p64["out_grad"].view
    need = _lib.lib().am_icp_workspace_bytes(P, Q, B)
    arenas["workspace"] = Arena.flat((need,), torch.uint8, dev)
    d.workspace = arenas["workspace"].view
    inputs = {"pred": Arena.flat_of(tp), "gt": Arena.flat_of(tg), "rot_init": Arena.flat_of(tr)}
    ops.icp_step(d, inputs["pred"].view, inputs["gt"].view, inputs["rot_init"].view, t=3, return_sums=True)
    for name, a in {**arenas, **inputs}.items():
        a.assert_untouched(name)
    for name, a in p64.items():
        a.assert_untouched(name, written=True)
    for name, a in inputs.items():
        assert same_bits(a.view, {"pred": tp, "gt": tg, "rot_init": tr}[name]), name
    for name in F32_FIELDS + ("out_sums", "out_grad"):
        assert same_bits(getattr(d, name), getattr(plain, name)), name
    assert int(d.out_flag.cpu()) == 0


# ------------------------------------------------------------------------------------------------------------------ 9. bad arguments
def test_bad_arguments_are_refused_before_any_launch(dev):
    pred, gt, rot, st = make_case(3, 37, 5)
    tp, tg, tr = to_dev(dev, pred, gt, rot)
    d = load(st, dev)
    ops.icp_step(d, tp, tg, tr, t=1, update=False)
    held = {name: getattr(d, name).clone() for name in F32_FIELDS}
    with pytest.raises(TypeError):
        ops.icp_step(d, tp.double(), tg, tr, t=1)
    with pytest.raises(TypeError):
        ops.icp_step(d, tp, tg, tr.half(), t=1)
    with pytest.raises(RuntimeError, match="device tensor"):
        ops.icp_step(d, tp.cpu(), tg, tr, t=1)
    for args in ((tp[:, :2].contiguous(), tg, tr), (tp, tg.reshape(1, -1, 3), tr), (tp[:0], tg, tr), (tp, tg, tr[:2]), (tp, tg, torch.cat((tr, tr))),
                 (tp.t(), tg, tr)):
        with pytest.raises(ValueError):
            ops.icp_step(d, *args, t=1)
    with pytest.raises(ValueError, match="step count"):
        ops.icp_step(d, tp, tg, tr, t=0)
    wrong = load(st, dev)
    wrong.params = wrong.params[:, :11].contiguous()
    with pytest.raises(ValueError, match="state.params"):
        ops.icp_step(wrong, tp, tg, tr, t=1)
    wrong = load(st, dev)
    wrong.adam_v = wrong.adam_v.double()
    with pytest.raises(TypeError):
        ops.icp_step(wrong, tp, tg, tr, t=1)
    small = d.workspace
    d.workspace = torch.empty((d.workspace_bytes - 8,), dtype=torch.uint8, device=dev)          # the caller's buffer, too small
    with pytest.raises(RuntimeError, match="workspace of"):
        ops.icp_step(d, tp, tg, tr, t=1)
    d.workspace = small
    torch.cuda.synchronize(dev)
    for name, val in held.items():                                                              # nothing ran
        assert same_bits(getattr(d, name), val), name
    ops.icp_step(d, tp, tg, tr, t=1)                                                            # and the state still serves
    assert not same_bits(d.params, held["params"])
