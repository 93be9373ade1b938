"""CPU suite of the WIDER FACE evaluator (dan_amd/wider_eval.py, csrc/wider_eval_exact.hip): the numpy restatement (tests/wider_protocol.py)
reproduces every hand-traced known answer; the ABI-5 symbols are declared, bound and exported by both builds; bad arguments are refused
before any launch; the ground-truth containers build the CSR arrays the kernels read."""
import ctypes
import io
import json
import os
import re

import numpy as np
import pytest
import torch

import wider_protocol as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "wider_kats.json")))["kats"]
NEW_SYMBOLS = ("danhip_wider_quantize", "danhip_wider_score_range", "danhip_wider_score_range_workspace_bytes", "danhip_wider_eval",
               "danhip_wider_eval_workspace_bytes", "danhip_wider_ap")


def kat_inputs(kat):
    """-> (dets per image as (x, y, w, h, score) float64 rows, boxes per image, keep per image [m,S]); a quantised KAT goes through
    eval_dan.write_to_txt and the text parser first."""
    from dan_amd.eval_dan import write_to_txt
    dets = []
    for i, im in enumerate(kat["images"]):
        d = np.asarray(im["dets"], dtype=np.float64).reshape(-1, 5)
        if kat["quantize"]:
            d = W.text_route(write_to_txt, d.astype(np.float32), "ev", "im%d" % i)
        dets.append(d)
    boxes = [np.asarray(im["boxes"], dtype=np.float64).reshape(-1, 4) for im in kat["images"]]
    keep = [np.asarray(im["keep"], dtype=np.uint8).reshape(len(b), kat["subsets"]) for im, b in zip(kat["images"], boxes)]
    return dets, boxes, keep


def kat_curves(kat, T=1000):
    c = np.zeros((kat["subsets"], T, 2), dtype=np.int64)
    for s, runs in enumerate(kat["expect"]["curve_runs"]):
        for a, b, c0, c1 in runs:
            c[s, a:b + 1] = (c0, c1)
    return c


@pytest.mark.parametrize("kat", KATS, ids=[k["name"] for k in KATS])
def test_restatement_reproduces_the_hand_traced_answers(kat):
    dets, boxes, keep = kat_inputs(kat)
    exp = kat["expect"]
    if "rows_after_text" in exp:
        for d, want in zip(dets, exp["rows_after_text"]):
            assert np.array_equal(d, np.asarray(want, dtype=np.float64).reshape(-1, 5))
    r = W.evaluate(dets, boxes, keep, kat["subsets"])
    assert (r["lo"], r["hi"]) == (exp["lo"], exp["hi"])
    assert r["count_face"].tolist() == exp["count_face"]
    for key, walk in exp["walks"].items():
        i, s = (int(v) for v in key.split(","))
        assert r["per_image"][(i, s)] == (walk["pred_recall"], walk["proposal"]), key
    assert np.array_equal(r["curves"], kat_curves(kat))
    assert np.abs(r["ap"] - np.asarray(exp["ap"])).max() <= 1e-12
    # a zero curve[t][0] gives precision 0 by definition, and the value never reaches the AP: replacing it by NaN's stand-in 1e9 at those
    # entries changes nothing (they sit at recall 0, in front of the envelope's first step)
    zero = r["curves"][..., 0] == 0
    assert (r["curves"][..., 1][zero] == 0).all() and (r["precision"][zero] == 0).all()


def test_kats_cover_the_cases_the_protocol_is_easy_to_get_wrong_on():
    names = {k["name"] for k in KATS}
    assert {"issue_example", "overlap_tie_first_index_wins", "score_tie_lower_index_first", "hi_equals_lo", "only_match_is_a_not_kept_box",
            "overlap_exactly_one_half", "text_route_three_filters"} <= names
    assert all(len(k["comment"]) > 80 for k in KATS)                 # each one carries its trace


def test_score_text_formula_is_the_formatted_text():
    """k = rint(double(score) * 1000) / 1000 (the kernel's formula) is the double that parsing '{:.3f}' gives: random fp32 scores and the
    half-way cases an fp32 can hold exactly."""
    rng = np.random.RandomState(0)
    s = np.concatenate([rng.rand(20000).astype(np.float32), (np.arange(1000, dtype=np.float64) / 1000 + 0.0005).astype(np.float32),
                        np.array([0.0625, 0.1875, 0.5625, 0.0005, 0.0015, 0.0025], dtype=np.float32)])
    want = np.array([float("{:.3f}".format(v)) for v in s])
    got = np.rint(s.astype(np.float64) * 1000.0) / 1000.0
    assert np.array_equal(got, want)


def test_new_symbols_are_declared_bound_and_exported_by_both_builds():
    from dan_amd import _lib, build
    build.build()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "danhip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(danhip_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    L16 = ctypes.CDLL(build.OUT_F16)
    for n in NEW_SYMBOLS:
        assert n in declared, n
        assert hasattr(L, n) and hasattr(L16, n), n
        if not n.endswith("_workspace_bytes"):
            assert n in _lib.SIGNATURES, n
    assert L.danhip_version() >= 5
    _lib.bind(L16, ["danhip_version"])
    assert L16.danhip_version() >= 5


def test_entry_points_refuse_bad_arguments_before_any_launch():
    from dan_amd import _lib
    L = _lib.lib()
    one = ctypes.c_void_p(64)                                         # never dereferenced: every check comes before the launch
    EINVAL, EWORKSPACE = -1, -3
    assert L.danhip_wider_quantize(None, 0, one, one, 1, 8, 1, one, one, 4, 8, one, None) == EINVAL and b"null" in L.danhip_last_error()
    assert L.danhip_wider_quantize(one, 0, one, one, 1, 8, 1, None, one, 4, 8, one, None) == EINVAL
    assert L.danhip_wider_quantize(one, 0, one, one, 1, 4096, 1, one, one, 4, 4096, one, None) == EINVAL and b"2048" in L.danhip_last_error()
    assert L.danhip_wider_quantize(one, 0, one, one, 1, 16, 1, one, one, 4, 8, one, None) == EINVAL          # Nmax above the store's rows per image
    assert L.danhip_wider_quantize(one, 4, one, one, 1, 8, 1, one, one, 4, 8, one, None) == EINVAL and b"fp32" in L.danhip_last_error()
    assert L.danhip_wider_score_range(one, 4, None, one, 1 << 20, None) == EINVAL
    assert L.danhip_wider_score_range(None, 4, one, one, 1 << 20, None) == EINVAL
    assert L.danhip_wider_score_range(one, 4, one, one, 8, None) == EWORKSPACE
    need = L.danhip_wider_eval_workspace_bytes(10, 3, 1000)
    assert need == 10 * 3 * 1000 * 2 * 4 and L.danhip_wider_eval_workspace_bytes(100000, 3, 1000) == 512 * 3 * 1000 * 2 * 4
    ok = (one, one, 5, one, one, one, 5, one, 10, 3, 1000, 2048, 0.5, one, need, one, None)
    for k in (0, 1, 3, 4, 5, 7, 13, 15):                              # each pointer in turn
        bad = list(ok)
        bad[k] = None
        assert L.danhip_wider_eval(*bad) == EINVAL, k
    bad = list(ok)
    bad[11] = 2049                                                    # a detection count above the kernel's bound
    assert L.danhip_wider_eval(*bad) == EINVAL and b"2048" in L.danhip_last_error()
    for k, v in ((8, 0), (9, 9), (10, 2047), (10, 0)):
        bad = list(ok)
        bad[k] = v
        assert L.danhip_wider_eval(*bad) == EINVAL, (k, v)
    bad = list(ok)
    bad[14] = need - 1
    assert L.danhip_wider_eval(*bad) == EWORKSPACE
    okap = (one, need, one, 5, 10, 3, 1000, one, one, one, one, one, None)
    for k in (0, 2, 7, 8, 9, 10, 11):
        bad = list(okap)
        bad[k] = None
        assert L.danhip_wider_ap(*bad) == EINVAL, k
    bad = list(okap)
    bad[1] = need - 1
    assert L.danhip_wider_ap(*bad) == EWORKSPACE


def test_ground_truth_builds_the_csr_arrays():
    from dan_amd.wider_eval import WiderGroundTruth
    gt = WiderGroundTruth([[[1, 2, 3, 4], [5, 6, 7, 8]], np.zeros((0, 4)), [[9, 10, 11, 12]]],
                          [[[1, 1, 1], [0, 1, 1]], np.zeros((0, 3)), [[0, 0, 1]]], names=["a/x", "a/y", "b/z"])
    assert gt.num_images == 3 and gt.offsets.dtype == np.int32 and gt.offsets.tolist() == [0, 2, 2, 3]
    assert gt.boxes.dtype == np.float64 and gt.boxes.tolist() == [[1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11, 12]]
    assert gt.keep.dtype == np.uint8 and gt.keep.tolist() == [7, 6, 4]
    assert gt.index_of("b/z") == 2 and gt.subsets == ("easy", "medium", "hard")
    b, k = gt.image(0)
    assert b.tolist() == [[1, 2, 3, 4], [5, 6, 7, 8]] and k.tolist() == [[1, 1, 1], [0, 1, 1]]
    with pytest.raises(ValueError):
        WiderGroundTruth([[[1, 2, 3, 4]]], [[[2]]], subsets=("all",))
    with pytest.raises(ValueError):
        WiderGroundTruth([[[1, 2, 3, 4]]], [[[1]]], subsets=tuple("abcdefghi"))


def test_evaluator_checks_its_arguments_on_the_host():
    from dan_amd import wider_eval
    gt = wider_eval.WiderGroundTruth([[[1, 2, 3, 4]]], [[[1]]], subsets=("all",))
    with pytest.raises(ValueError):
        wider_eval.WiderEvaluator(gt, max_per_image=4096, device="cpu")
    with pytest.raises(ValueError):
        wider_eval.WiderEvaluator(gt, thresholds=5000, device="cpu")
    ev = wider_eval.WiderEvaluator(gt, max_per_image=8, device="cpu")
    with pytest.raises(ValueError):
        ev.add([0], torch.zeros((1, 9, 5)), torch.zeros((1,), dtype=torch.int32))          # more rows than the store holds per image
    with pytest.raises(IndexError):
        ev.add([3], torch.zeros((1, 4, 5)), torch.zeros((1,), dtype=torch.int32))
    with pytest.raises(ValueError):
        ev.add([0, 0], torch.zeros((2, 4, 5)), torch.zeros((2,), dtype=torch.int32))


def test_pred_text_parsers_agree_and_read_a_directory(tmp_path):
    from dan_amd import wider_eval
    from dan_amd.eval_dan import write_to_txt
    rng = np.random.RandomState(3)
    want = {}
    for e, n in (("0--Parade", "0_Parade_a_1"), ("0--Parade", "0_Parade_b_2"), ("12--Group", "12_Group_c_3")):
        xy = rng.rand(30, 2).astype(np.float32) * 300
        wh = rng.rand(30, 2).astype(np.float32) * 60
        det = np.concatenate([xy, xy + wh, rng.rand(30, 1).astype(np.float32)], axis=1)
        os.makedirs(tmp_path / e, exist_ok=True)
        with open(tmp_path / e / (n + ".txt"), "w") as f:
            write_to_txt(f, det, e, n)
        f = io.StringIO()
        write_to_txt(f, torch.from_numpy(det), e, n)
        want[e + "/" + n] = W.parse_pred_text(f.getvalue())[e + "/" + n]
    got = wider_eval.read_pred_dir(str(tmp_path))
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == np.float64 and np.array_equal(got[k], want[k]) and 0 < got[k].shape[0] < 30


def test_mat_loader_round_trips_a_synthetic_annotation_file(tmp_path):
    sio = pytest.importorskip("scipy.io")
    from dan_amd.wider_eval import WiderGroundTruth
    rng = np.random.RandomState(1)
    events = ["0--Parade", "1--Handshaking"]
    files = [["0_Parade_a_1", "0_Parade_b_2", "0_Parade_c_3"], ["1_Handshaking_d_4"]]

    def cell(items):
        c = np.empty((len(items), 1), dtype=object)
        for i, v in enumerate(items):
            c[i, 0] = v
        return c

    boxes, kept = [], [[], [], []]
    for fl in files:
        eb, ek = [], [[], [], []]
        for _ in fl:
            n = int(rng.randint(1, 6))
            eb.append(rng.randint(0, 500, (n, 4)).astype(np.float64))
            hard = np.sort(rng.choice(n, size=int(rng.randint(1, n + 1)), replace=False)) + 1
            medium, easy = hard[:max(1, len(hard) - 1)], hard[:1]
            for s, idx in enumerate((easy, medium, hard)):
                ek[s].append(idx.reshape(-1, 1).astype(np.float64))
        boxes.append(eb)
        for s in range(3):
            kept[s].append(ek[s])
    sio.savemat(str(tmp_path / "split.mat"), {"event_list": cell(events), "file_list": cell([cell(f) for f in files]),
                                               "face_bbx_list": cell([cell(b) for b in boxes])})
    for s, n in enumerate(("easy", "medium", "hard")):
        sio.savemat(str(tmp_path / (n + ".mat")), {"gt_list": cell([cell(k) for k in kept[s]])})
    gt = WiderGroundTruth.from_mat(*(str(tmp_path / n) for n in ("split.mat", "easy.mat", "medium.mat", "hard.mat")))
    assert gt.names == ["0--Parade/0_Parade_a_1", "0--Parade/0_Parade_b_2", "0--Parade/0_Parade_c_3", "1--Handshaking/1_Handshaking_d_4"]
    flat = [b for eb in boxes for b in eb]
    assert gt.offsets.tolist() == np.concatenate([[0], np.cumsum([len(b) for b in flat])]).tolist()
    assert np.array_equal(gt.boxes, np.concatenate(flat))
    i = 0
    for e in range(len(events)):
        for f in range(len(files[e])):
            _, k = gt.image(i)
            for s in range(3):
                assert (np.nonzero(k[:, s])[0] + 1).tolist() == kept[s][e][f].reshape(-1).astype(int).tolist()
            i += 1
