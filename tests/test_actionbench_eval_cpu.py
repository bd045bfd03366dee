"""The ActionBench dataset evaluator (actionmesh_amd.actionbench, the mirror of the reference's evaluate_dataset.py) without a GPU:
discovery, natural order, truncation, file formats, resumption - through an injected metrics function."""
import csv
import json
import math

import numpy as np
import pytest

from actionmesh_amd import actionbench as AB
from actionmesh_amd import mesh_io

TET_V = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
TET_F = np.int64([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])


def make_dataset(root, uids=("b_10", "a_2"), frames=3, meshes=None):
    gt, pred = root / "gt", root / "pred"
    for uid in uids:
        (gt / uid).mkdir(parents=True)
        np.save(gt / uid / "surfaces.npy", np.random.RandomState(0).rand(frames, 50, 6).astype(np.float32))
        (pred / uid).mkdir(parents=True)
        for t in range(frames if meshes is None else meshes):
            mesh_io.save_glb(TET_V * (t + 1), TET_F, pred / uid / f"mesh_{t}.glb")
    return gt, pred


class Metrics:
    """records its calls; the metrics are functions of the first mesh's scale, so they tell which files were handed over"""

    def __init__(self, fail=()):
        self.calls, self.fail = [], set(fail)

    def __call__(self, gt_pc, pred_meshes, device, is_4D, n_pts_icp, n_pts_chamfer, seed, n_iter, nn):
        self.calls.append(dict(frames=len(pred_meshes), gt=tuple(gt_pc.shape), is_4D=is_4D, n_pts_icp=n_pts_icp, n_pts_chamfer=n_pts_chamfer,
                               seed=seed, n_iter=n_iter, nn=nn, scales=[float(v[:, 0].max()) for v, _ in pred_meshes]))
        if len(self.calls) in self.fail:
            raise RuntimeError("metrics failed")
        return 1.5, 2.5, (0.25 if is_4D else 0.0)


def test_find_uids_and_its_three_errors(tmp_path):
    gt, pred = make_dataset(tmp_path)
    assert AB.find_uids(gt, pred) == ["a_2", "b_10"]
    (gt / "only_gt").mkdir()
    np.save(gt / "only_gt" / "surfaces.npy", np.zeros((1, 4, 3), np.float32))
    (pred / "only_pred").mkdir()
    mesh_io.save_glb(TET_V, TET_F, pred / "only_pred" / "mesh_0.glb")
    assert AB.find_uids(gt, pred) == ["a_2", "b_10"]
    assert AB.find_uids(gt, pred, mesh_pattern="*.glb") == ["a_2", "b_10"]
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(FileNotFoundError, match="No GT samples"):
        AB.find_uids(empty, pred)
    with pytest.raises(FileNotFoundError, match="No predictions"):
        AB.find_uids(gt, empty)
    with pytest.raises(FileNotFoundError, match="No predictions"):
        AB.find_uids(gt, pred, mesh_pattern="frame_*.obj")
    other = tmp_path / "other"
    (other / "zzz").mkdir(parents=True)
    mesh_io.save_glb(TET_V, TET_F, other / "zzz" / "mesh_0.glb")
    with pytest.raises(ValueError, match="No common UIDs"):
        AB.find_uids(gt, other)


def test_natural_order_truncation_and_round_trip(tmp_path):
    d = tmp_path / "m"
    d.mkdir()
    for t in (10, 2, 0, 1, 11):
        mesh_io.save_glb(TET_V * (t + 1), TET_F, d / f"mesh_{t}.glb")
    names = sorted((p.name for p in d.glob("mesh_*.glb")), key=AB.natural_key)
    assert names == ["mesh_0.glb", "mesh_1.glb", "mesh_2.glb", "mesh_10.glb", "mesh_11.glb"]            # mesh_2 before mesh_10
    assert sorted(["a10b", "a2b", "A1", "a2a"], key=AB.natural_key) == ["A1", "a2a", "a2b", "a10b"]
    meshes = AB.load_pred_meshes(d)
    assert [float(v[:, 0].max()) for v, _ in meshes] == [1.0, 2.0, 3.0, 11.0, 12.0]
    for t, (v, f) in zip((0, 1, 2, 10, 11), meshes):              # save_glb -> load_pred_meshes round trip, bit for bit
        assert v.dtype == np.float32 and f.dtype == np.int64 and np.array_equal(v, TET_V * (t + 1)) and np.array_equal(f, TET_F)
    assert [float(v[:, 0].max()) for v, _ in AB.load_pred_meshes(d, n_frames=3)] == [1.0, 2.0, 3.0]      # truncation to the first n
    with pytest.raises(ValueError, match="Not enough meshes: found 5, need 6"):
        AB.load_pred_meshes(d, n_frames=6)
    with pytest.raises(FileNotFoundError, match="No mesh files"):
        AB.load_pred_meshes(d, pattern="nothing_*.glb")
    assert tuple(AB.load_gt_surfaces(make_dataset(tmp_path / "ds")[0] / "a_2" / "surfaces.npy").shape) == (3, 50, 3)


def test_evaluate_sample_statuses(tmp_path):
    gt, pred = make_dataset(tmp_path, frames=3, meshes=5)
    m = Metrics()
    r = AB.evaluate_sample("a_2", gt, pred, _metrics=m, n_iter=7, nn="grid")
    assert (r.status, r.n_frames, r.cd_3d, r.cd_4d, r.cd_motion, r.error_message) == ("success", 3, 1.5, 2.5, 0.25, "")
    assert m.calls[0]["frames"] == 3 and m.calls[0]["scales"] == [1.0, 2.0, 3.0] and m.calls[0]["gt"] == (3, 50, 3)
    assert (m.calls[0]["n_pts_icp"], m.calls[0]["n_pts_chamfer"], m.calls[0]["seed"], m.calls[0]["n_iter"], m.calls[0]["nn"]) == (10_000, 100_000, 44, 7, "grid")
    assert AB.evaluate_sample("a_2", gt, pred, is_4d=False, _metrics=m).cd_motion == 0.0
    r = AB.evaluate_sample("nobody", gt, pred, _metrics=m)
    assert r.status == "error" and "GT not found" in r.error_message
    gt2, pred2 = make_dataset(tmp_path / "short", frames=4, meshes=2)
    r = AB.evaluate_sample("a_2", gt2, pred2, _metrics=m)
    assert r.status == "error" and r.error_message == "Not enough meshes: found 2, need 4" and r.n_frames == 4
    (pred / "a_2" / "mesh_1.glb").write_bytes(b"not a glb at all, but long enough")          # what load_glb cannot read is the sample's error
    r = AB.evaluate_sample("a_2", gt, pred, _metrics=m)
    assert r.status == "error" and "GLB" in r.error_message
    r = AB.evaluate_sample("b_10", gt, pred, _metrics=Metrics(fail={1}))
    assert r.status == "error" and r.error_message == "metrics failed" and math.isnan(r.cd_3d)


def test_csv_summary_resume_recompute_and_retry(tmp_path):
    gt, pred = make_dataset(tmp_path, uids=("u1", "u2", "u3"))
    out = tmp_path / "res" / "results.csv"
    m = Metrics(fail={2})
    res = AB.evaluate_dataset(str(gt), str(pred), output_csv=str(out), _metrics=m, n_pts_icp=11, n_pts_chamfer=22, seed=5)
    assert len(m.calls) == 3 and [s.status for s in res.samples] == ["success", "error", "success"]
    assert m.calls[0]["n_pts_icp"] == 11 and m.calls[0]["n_pts_chamfer"] == 22 and m.calls[0]["seed"] == 5 and m.calls[0]["is_4D"]
    with open(out, newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["uid", "cd_3d", "cd_4d", "cd_motion", "n_frames", "status", "error_message"] == AB.CSV_COLUMNS      # the dataclass's order
    assert rows[1] == ["u1", "1.5", "2.5", "0.25", "3", "success", ""] and rows[2] == ["u2", "", "", "", "3", "error", "metrics failed"]
    summary = json.loads(out.with_suffix(".summary.json").read_text())
    assert list(summary) == ["n_total", "n_success", "n_failed", "success_rate", "cd_3d_mean", "cd_4d_mean", "cd_motion_mean"]
    assert summary["n_total"] == 3 and summary["n_success"] == 2 and summary["n_failed"] == 1 and summary["success_rate"] == 2 / 3
    assert (summary["cd_3d_mean"], summary["cd_4d_mean"], summary["cd_motion_mean"]) == (1.5, 2.5, 0.25)
    loaded = AB.load_existing_results(out)
    assert list(loaded) == ["u1", "u2", "u3"] and loaded["u1"] == res.samples[0] and loaded["u2"].status == "error"
    assert math.isnan(loaded["u2"].cd_3d) and loaded["u2"].error_message == "metrics failed" and loaded["u3"].n_frames == 3
    # resume: the successful rows are taken over, the failed one is retried
    m2 = Metrics()
    res2 = AB.evaluate_dataset(str(gt), str(pred), output_csv=str(out), _metrics=m2)
    assert len(m2.calls) == 1 and [s.status for s in res2.samples] == ["success"] * 3 and [s.uid for s in res2.samples] == ["u1", "u2", "u3"]
    # a second call computes nothing
    m3 = Metrics()
    AB.evaluate_dataset(str(gt), str(pred), output_csv=str(out), _metrics=m3)
    assert m3.calls == []
    # --recompute redoes all
    m4 = Metrics()
    AB.evaluate_dataset(str(gt), str(pred), output_csv=str(out), recompute=True, _metrics=m4)
    assert len(m4.calls) == 3
    # no CSV: nothing is written, everything is computed
    m5 = Metrics()
    assert AB.evaluate_dataset(str(gt), str(pred), _metrics=m5).summary()["n_success"] == 3 and len(m5.calls) == 3
    assert AB.load_existing_results(tmp_path / "none.csv") == {}
    empty = AB.DatasetResults().summary()
    assert empty["n_total"] == 0 and empty["success_rate"] == 0.0 and math.isnan(empty["cd_3d_mean"])


def test_cli_flags(tmp_path, monkeypatch, capsys):
    gt, pred = make_dataset(tmp_path)
    seen = {}

    def fake(**kw):
        seen.update(kw)
        r = AB.DatasetResults()
        r.add(AB.SampleResult("a_2", 1.0, 2.0, 3.0, 3, "success", ""))
        r.add(AB.SampleResult("b_10", status="error", error_message="boom"))
        return r

    monkeypatch.setattr(AB, "evaluate_dataset", fake)
    AB.main(["--gt_root", str(gt), "--pred_root", str(pred), "--output_csv", "x.csv", "--n_pts_icp", "7", "--n_pts_chamfer", "9", "--seed", "3",
             "--mesh_pattern", "*.glb", "--recompute", "--3d-only", "--nn", "grid", "--n_iter", "5", "--device", "cuda:0"])
    assert seen == dict(gt_root=str(gt), pred_root=str(pred), output_csv="x.csv", device="cuda:0", n_pts_icp=7, n_pts_chamfer=9, seed=3,
                        mesh_pattern="*.glb", recompute=True, is_4d=False, n_iter=5, nn="grid")
    text = capsys.readouterr().out
    assert "EVALUATION SUMMARY" in text and "Rate:    50.0%" in text and "CD_Motion: 3.000" in text and "[b_10] error: boom" in text
    seen.clear()
    AB.main(["--gt_root", "g", "--pred_root", "p"])
    assert seen["nn"] == AB.EVALUATOR_NN and seen["n_iter"] == 200 and seen["n_pts_chamfer"] == 100_000 and seen["is_4d"] and not seen["recompute"]


def test_nn_keyword_is_validated():
    import torch
    with pytest.raises(ValueError, match="nn must be"):
        AB.chamfer_distance_sq(torch.zeros(1, 2, 3), torch.zeros(1, 2, 3), nn="kdtree")
    with pytest.raises(ValueError, match="nn must be"):
        AB.gradient_icp(torch.zeros(2, 3), torch.zeros(2, 3), nn="kdtree")
