"""The fused ICP iteration without a GPU: the numpy restatement of am_icp_step's contract (tests/_icp_ref.py) against the oracle's
autograd path and torch.optim.Adam, the new keywords of actionbench, the binding's tables, and the C-ABI's argument checks (which
refuse before anything is launched)."""
import ctypes

import numpy as np
import pytest
import torch

import _icp_ref as REF
from actionmesh_amd import _lib, actionbench as AB
from oracle import actionbench_oracle as O

B, P, Q = 24, 400, 350
EPS32 = 2.0 ** -24


@pytest.fixture(scope="module")
def case():
    """a perturbed, non-identity state with a non-trivial Adam history, the restatement's step from it (t = 3) and the oracle's
    autograd gradients at the same point"""
    rng = np.random.default_rng(11)
    pred = rng.standard_normal((P, 3)).astype(np.float32) * np.float32([1.0, 0.6, 0.3])
    gt = rng.standard_normal((Q, 3)).astype(np.float32) * np.float32([0.9, 0.7, 0.4]) + np.float32([0.1, -0.05, 0.02])
    rot_init = O.canonical_rotation_matrices().numpy().reshape(B, 9)
    st = REF.State(B)
    st.params = (st.params + 0.1 * rng.standard_normal((B, 12))).astype(np.float32)
    st.adam_m = (1e-2 * rng.standard_normal((B, 12))).astype(np.float32)
    st.adam_v = (1e-4 * rng.standard_normal((B, 12)) ** 2).astype(np.float32)
    before = st.copy()
    sums, mags, counts, flag = REF.sums_of(pred, gt, st.params, rot_init)
    assert flag == 0 and (counts == [P, Q]).all()
    REF.step(st, pred, gt, rot_init, t=3)
    # the oracle: autograd through the min, the reference's loss.mean().backward()
    T = torch.nn.Parameter(torch.from_numpy(before.params[:, 0:3].copy()))
    R6 = torch.nn.Parameter(torch.from_numpy(before.params[:, 3:9].copy()))
    s = torch.nn.Parameter(torch.from_numpy(before.params[:, 9:12].copy()))
    with torch.enable_grad():
        R = torch.from_numpy(rot_init).reshape(B, 3, 3) @ O.rotation_6d_to_matrix(R6)
        loss = O.chamfer_distance_sq(s[:, None] * torch.from_numpy(pred)[None] @ R + T[:, None], torch.from_numpy(gt)[None].expand(B, -1, -1))
        loss.mean().backward()
    # the fp32 summation bound of the autograd side, per sum: 2 N 2^-24 sum|terms| from the restatement's own terms; the gradient is
    # linear in the sums, so the bound of an entry is |J| . bound, J column by column from the restatement's own chain rule
    n = np.array([P, Q], np.float64)[None, :, None]
    sum_bound = 2.0 * n * EPS32 * mags
    g_bound, loss_bound = np.empty((B, 12)), np.empty(B)
    for b in range(B):
        J = REF.jacobian(before.params[b], rot_init[b], P, Q, B)
        bound = np.abs(J) @ sum_bound[b].reshape(26)
        loss_bound[b], g_bound[b] = bound[0], bound[1:]
    return dict(pred=pred, gt=gt, rot_init=rot_init, before=before, after=st, loss=loss.detach().numpy(), T=T, R6=R6, s=s,
                g_bound=g_bound, loss_bound=loss_bound)


def test_restatement_matches_the_oracles_autograd(case):
    st = case["after"]
    g_ref = np.concatenate((case["T"].grad.numpy(), case["R6"].grad.numpy(), case["s"].grad.numpy()), axis=1).astype(np.float64)
    err = np.abs(st.out_grad - g_ref)
    print(f"gradient: max |diff| {err.max():.3e} on max |g| {np.abs(g_ref).max():.3e}; smallest bound {case['g_bound'].min():.3e}, "
          f"worst diff / bound {(err / case['g_bound']).max():.3e}")
    assert (err <= case["g_bound"]).all()
    lerr = np.abs(st.out_loss.astype(np.float64) - case["loss"].astype(np.float64))
    # the loss is stored in fp32 on both sides: one rounding each on top of the summation bound
    lbound = case["loss_bound"] + 2 * EPS32 * np.abs(case["loss"])
    print(f"loss: max relative diff {(lerr / case['loss']).max():.3e}, worst diff / bound {(lerr / lbound).max():.3e}")
    assert (lerr <= lbound).all()


def test_restatement_adam_step_matches_torch_adam(case):
    """one step (t = 3) from a non-trivial (m, v): the parameters against torch.optim.Adam fed the ORACLE's gradients.  Tolerance: the
    gradient bound pushed through the update, lr / bc1 |d(m' / denom) / dg| bound, plus what fp32 storage adds whatever the
    gradients are: torch forms m', v', the quotient and the new parameter in fp32 (a rounding each on an update of magnitude
    |delta|: 4 x 2^-24 |delta|) and both sides round the parameter itself (2 x 2^-24 |param|)."""
    before, after = case["before"], case["after"]
    params = [case["T"], case["R6"], case["s"]]
    cols = [slice(0, 3), slice(3, 9), slice(9, 12)]
    opt = torch.optim.Adam(params, lr=0.01)
    for p, c in zip(params, cols):
        opt.state[p] = {"step": torch.tensor(2.0), "exp_avg": torch.from_numpy(before.adam_m[:, c].copy()),
                        "exp_avg_sq": torch.from_numpy(before.adam_v[:, c].copy())}
    opt.step()
    got_ref = np.concatenate([p.detach().numpy() for p in params], axis=1).astype(np.float64)
    lr, b1, b2, eps, t = 0.01, 0.9, 0.999, 1e-8, 3
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    g = after.out_grad
    m2 = b1 * before.adam_m.astype(np.float64) + (1 - b1) * g
    v2 = b2 * before.adam_v.astype(np.float64) + (1 - b2) * g * g
    root = np.sqrt(v2)
    denom = root / np.sqrt(bc2) + eps
    dq_dg = (1 - b1) / denom + np.abs(m2) * (1 - b2) * np.abs(g) / (root * np.sqrt(bc2) * denom ** 2)
    delta = lr / bc1 * np.abs(m2) / denom
    tol = lr / bc1 * dq_dg * case["g_bound"] + 4 * EPS32 * delta + 2 * EPS32 * np.abs(got_ref)
    err = np.abs(after.params.astype(np.float64) - got_ref)
    print(f"parameters: max |diff| {err.max():.3e}, worst diff / tolerance {(err / tol).max():.3e}, largest update {delta.max():.3e}")
    assert (err <= tol).all()
    assert np.abs(after.params - before.params).max() > 1e-3          # the step moved something
    for name in ("adam_m", "adam_v"):
        ref = np.concatenate([opt.state[p]["exp_avg" if name == "adam_m" else "exp_avg_sq"].numpy() for p in params], axis=1)
        assert np.allclose(getattr(after, name), ref, rtol=1e-4, atol=1e-9)


def test_best_so_far_rule_of_the_restatement(case):
    """pre-update R, post-update T and s of the lowest-index smallest loss; no change unless strictly lower"""
    before, after = case["before"], case["after"]
    c = int(np.argmin(after.out_loss))
    assert np.array_equal(after.best[:9], after.out_rot[c]) and after.best[15] == after.out_loss[c]
    assert np.array_equal(after.best[9:12], after.params[c, 0:3]) and np.array_equal(after.best[12:15], after.params[c, 9:12])
    assert not np.array_equal(after.params[c, 0:3], before.params[c, 0:3])
    st = after.copy()
    st.best[15] = after.best[15]                                     # equal is not strictly lower
    held = st.best.copy()
    st.params, st.adam_m, st.adam_v = before.params.copy(), before.adam_m.copy(), before.adam_v.copy()
    REF.step(st, case["pred"], case["gt"], case["rot_init"], t=3)
    assert np.array_equal(st.best, held)


def test_restatement_without_a_finite_distance():
    pred = np.float32([[0, 0, 0], [1, 0, 0], [np.nan, 0, 0]])
    gt = np.float32([[0, 0, 1], [1, 0, 1]])
    st = REF.State(2)
    sums, mags, counts, flag = REF.sums_of(pred, gt, st.params, np.tile(np.eye(3, dtype=np.float32).reshape(9), (2, 1)))
    assert flag == REF.NO_NEIGHBOUR and (counts == [2, 2]).all() and np.isfinite(sums).all() and sums[0, 0, 0] == 2.0
    assert np.array_equal(REF.match(np.float32([[0, 0, 0]]), np.float32([[1, 0, 0], [-1, 0, 0], [np.inf, 0, 0]])), [0])      # a tie: lowest index


def test_keywords_are_validated():
    z = torch.zeros(2, 3)
    with pytest.raises(ValueError, match="step must be"):
        AB.gradient_icp(z, z, step="bogus")
    with pytest.raises(ValueError, match="fused"):
        AB.gradient_icp(z, z, step="fused", nn="grid")
    with pytest.raises(ValueError, match="fused"):
        AB.gradient_icp(z, z, step="fused", _chamfer=lambda x, y: x)
    assert AB.ICP_STEPS == ("autograd", "fused") and AB.EVALUATOR_ICP == "autograd"
    with pytest.raises(ValueError, match="icp must be"):
        AB.evaluate_dataset("nowhere", "nowhere", icp="bogus")


def test_icp_keyword_reaches_the_metrics(tmp_path, monkeypatch):
    seen = []
    monkeypatch.setattr(AB, "evaluate_dataset", lambda **kw: seen.append(kw) or AB.DatasetResults())
    AB.main(["--gt_root", "g", "--pred_root", "p", "--icp", "fused"])
    AB.main(["--gt_root", "g", "--pred_root", "p"])
    assert seen[0]["icp"] == "fused" and "icp" not in seen[1]       # the default call is the one it was
    with pytest.raises(SystemExit):
        AB.main(["--gt_root", "g", "--pred_root", "p", "--icp", "bogus"])
    calls = []

    def metrics(**kw):
        calls.append(kw)
        return 1.0, 2.0, 3.0

    (tmp_path / "gt" / "u").mkdir(parents=True)
    np.save(tmp_path / "gt" / "u" / "surfaces.npy", np.zeros((1, 5, 3), np.float32))
    from actionmesh_amd import mesh_io
    (tmp_path / "pred" / "u").mkdir(parents=True)
    mesh_io.save_glb(np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]]), np.int64([[0, 1, 2]]), tmp_path / "pred" / "u" / "mesh_0.glb")
    monkeypatch.undo()
    res = AB.evaluate_dataset(str(tmp_path / "gt"), str(tmp_path / "pred"), _metrics=metrics, icp="fused")
    assert res.samples[0].status == "success" and calls[0]["icp"] == "fused"
    AB.evaluate_sample("u", tmp_path / "gt", tmp_path / "pred", _metrics=metrics)
    assert "icp" not in calls[1]


def test_binding_tables_hold_the_icp_entry():
    assert "am_icp_args" in _lib.STRUCTS and _lib.STRUCTS["am_icp_args"] is _lib.AmIcpArgs
    assert "am_icp_step" in _lib.SYMBOLS and "am_icp_workspace_bytes" in _lib.SYMBOLS
    assert _lib.ICP_NO_NEIGHBOUR == REF.NO_NEIGHBOUR == 1


def test_icp_argument_validation_without_gpu():
    """every refusal comes before a launch: the pointers below are never followed"""
    lib = _lib.lib()
    assert lib.am_icp_step(None, None, 0, None) != 0 and b"null arguments" in lib.am_last_error()
    buf = (ctypes.c_uint8 * 64)()
    ptr = (ctypes.addressof(buf) + 15) & ~15

    def args(**kw):
        a = _lib.AmIcpArgs()
        for name, _t in _lib.AmIcpArgs._fields_:
            if _t is ctypes.c_void_p and name not in ("out_sums", "out_grad"):
                setattr(a, name, ptr)
        a.n_pred, a.n_gt, a.batch, a.update = 1000, 700, 24, 1
        a.lr, a.beta1, a.beta2, a.eps, a.bias_correction1, a.bias_correction2 = 0.01, 0.9, 0.999, 1e-8, 0.1, 0.001
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    need = lib.am_icp_workspace_bytes(1000, 700, 24)
    assert need == 8 * 13 * 24 * (4 + 3) + 8 * 26 * 24            # a (13) partial per workgroup of 256 queries, then the (B, 2, 13) sums
    assert lib.am_icp_workspace_bytes(0, 5, 1) == 0 and lib.am_icp_workspace_bytes(5, 5, 0) == 0 and lib.am_icp_workspace_bytes(1 << 31, 5, 1) == 0
    assert lib.am_icp_workspace_bytes(5, 5, 65536) == 0
    for change, word in ((dict(n_pred=0), b"empty"), (dict(n_gt=0), b"empty"), (dict(batch=0), b"empty"), (dict(n_pred=1 << 31), b"32-bit"),
                         (dict(n_gt=1 << 31), b"32-bit"), (dict(batch=65536), b"z extent"), (dict(pred=None), b"null pointer"),
                         (dict(best=None), b"null pointer"), (dict(out_flag=None), b"null pointer"), (dict(bias_correction1=0.0), b"bias"),
                         (dict(out_sums=ptr + 4), b"aligned")):
        assert lib.am_icp_step(ctypes.byref(args(**change)), ptr, need, None) != 0, change
        msg = lib.am_last_error()
        assert msg.startswith(b"am_icp_step:") and word in msg, (change, msg)
    assert lib.am_icp_step(ctypes.byref(args()), ptr, need - 1, None) != 0 and b"workspace" in lib.am_last_error()
    assert lib.am_icp_step(ctypes.byref(args()), None, need, None) != 0 and b"workspace" in lib.am_last_error()
    assert lib.am_icp_step(ctypes.byref(args()), ptr + 4, need, None) != 0 and b"aligned" in lib.am_last_error()
