"""The evaluation command without a GPU (dan_amd/eval_cli.py): the flag blocks of the four reference scripts, the two routes to the file
list, eval_pb's row filter, and the drawing rule's numpy restatement (dan_amd/utility/draw_toolbox.py draw_reference - what the kernel is
compared with on the GPU) on hand-traced 12 x 12 cases."""
import io
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "eval_flags.json")))
MODELS = ("sfd", "pb", "dan", "dan_deform")


def test_flag_defaults_equal_the_reference_scripts():
    """tests/golden/eval_flags.json: names, order and default values of every tf.app.flags definition of the four evaluation scripts."""
    from dan_amd import eval_cli
    assert sorted(GOLDEN) == sorted(MODELS)
    for model in MODELS:
        d = eval_cli.flag_defaults(model)
        assert list(d.items()) == list(GOLDEN[model].items()), model
        args = eval_cli.build_parser(model).parse_args([])
        for name, value in GOLDEN[model].items():
            assert getattr(args, name) == value and type(getattr(args, name)) is type(value), (model, name)
        assert (args.device, args.precision, args.batch_images, args.decode_entropy, args.image_list, args.gt_dir, args.debug_quality) == \
            ("cuda:0", "act", 8, "host", None, None, 75)


def test_help_names_the_ignored_flags():
    from dan_amd import eval_cli
    text = eval_cli.build_parser("dan").format_help()
    for name in ("data_format", "num_classes", "train_image_size"):
        assert name in eval_cli.IGNORED_FLAGS
        at = text.index("--%s " % name, text.index("options:"))
        assert "ignored" in " ".join(text[at:at + 300].split()[:14]), name
    args = eval_cli.build_parser("dan").parse_args(["--data_format", "channels_first", "--num_classes", "3", "--train_image_size", "512"])
    assert args.train_image_size == 512


def test_every_model_has_a_command():
    import importlib
    for model in MODELS:
        m = importlib.import_module("dan_amd.eval_%s" % model)
        assert callable(m.main) and callable(m.write_to_txt) and callable(m.detect_image)


def test_image_list_route(tmp_path):
    from dan_amd import eval_cli
    p = tmp_path / "list.txt"
    p.write_text("# val\n0--Parade/0_Parade_a\n1--Handshaking/1_x.jpg\n\n0--Parade/0_Parade_b\n")
    assert eval_cli.read_image_list(str(p)) == [("0--Parade", ["0_Parade_a", "0_Parade_b"]), ("1--Handshaking", ["1_x"])]
    (tmp_path / "bad.txt").write_text("no_event\n")
    with pytest.raises(ValueError):
        eval_cli.read_image_list(str(tmp_path / "bad.txt"))


def test_mat_route_yields_the_same_list(tmp_path):
    sio = pytest.importorskip("scipy.io")
    from dan_amd import eval_cli
    events = [("0--Parade", ["0_Parade_a", "0_Parade_b", "0_Parade_c"]), ("1--Handshaking", ["1_x"])]
    event_list = np.empty((len(events), 1), dtype=object)
    file_list = np.empty((len(events), 1), dtype=object)
    for e, (event, names) in enumerate(events):
        event_list[e, 0] = np.array([event])
        cell = np.empty((len(names), 1), dtype=object)
        for i, n in enumerate(names):
            cell[i, 0] = np.array([n])
        file_list[e, 0] = cell
    split = tmp_path / "wider_face_split"
    split.mkdir()
    sio.savemat(str(split / "wider_face_val.mat"), {"event_list": event_list, "file_list": file_list})
    (tmp_path / "list.txt").write_text("".join("%s/%s\n" % (e, n) for e, names in events for n in names))
    by_mat = eval_cli.file_list(eval_cli.build_parser("sfd").parse_args(["--data_dir", str(tmp_path)]))
    by_list = eval_cli.file_list(eval_cli.build_parser("sfd").parse_args(["--data_dir", str(tmp_path), "--image_list", str(tmp_path / "list.txt")]))
    assert by_mat == by_list == events


def test_eval_pb_writes_the_row_eval_dan_drops():
    """A detection 9.5 px high: ceil(9.5) = 10 passes both filters, so the row that tells them apart is ceil(height) = 9, i.e. ymax - ymin + 1
    in (8, 9]; the 9.5 px row is written by both, the 8.5 px row by eval_pb alone."""
    from dan_amd import eval_dan, eval_pb
    det = np.array([[10.0, 20.0, 30.0, 28.5, 0.9],        # height 9.5 -> ceil 10
                    [40.0, 20.0, 60.0, 27.5, 0.8],        # height 8.5 -> ceil 9
                    [70.0, 20.0, 90.0, 26.5, 0.7]], np.float32)   # height 7.5 -> ceil 8
    a, b = io.StringIO(), io.StringIO()
    eval_dan.write_to_txt(a, det, "ev", "im")
    eval_pb.write_to_txt(b, det, "ev", "im")
    assert a.getvalue() == "ev/im.jpg\n1\n10.0 20.0 21.0 10.0 0.900\n"
    assert b.getvalue() == "ev/im.jpg\n2\n10.0 20.0 21.0 10.0 0.900\n40.0 20.0 21.0 9.0 0.800\n"


def test_written_rows_restates_write_to_txt():
    from dan_amd import eval_cli, eval_dan
    from dan_amd.wider_eval import parse_pred_text
    rng = np.random.RandomState(3)
    xy = rng.rand(40, 2) * 200
    wh = rng.rand(40, 2) * 24
    det = np.concatenate([xy, xy + wh, rng.rand(40, 1) * 0.05], 1).astype(np.float32)
    for min_height in (9, 10):
        f = io.StringIO()
        eval_dan.write_to_txt(f, det, "ev", "im", 0.01, min_height=min_height)
        assert np.array_equal(parse_pred_text(f.getvalue())["ev/im"], eval_cli.written_rows(det, 0.01, min_height))


# ------------------------------------------------------------------------------------------------- the drawing rule, traced by hand
def _mask(rows):
    assert len(rows) == 12 and all(len(r) == 12 for r in rows)
    return np.array([[c == "#" for c in r] for r in rows])


E = "............"
TRACED = [
    # a box inside the image: (3.7, 4.2, 8.9, 7.0) -> corners 3, 4, 8, 7; band x 2..9 / y 3..8 around the interior x 4..7 / y 5..6
    ("inside", [[3.7, 4.2, 8.9, 7.0]], [1],
     [E, E, E, "..########..", "..########..", "..##....##..", "..##....##..", "..########..", "..########..", E, E, E]),
    # clipped at the left and top borders: int() truncates toward zero, (-3.5, -2.2) -> (-3, -2); band x -4..5 / y -3..4, interior x -2..3 / y -1..2
    ("left_top", [[-3.5, -2.2, 4.0, 3.0]], [1],
     ["....##......", "....##......", "....##......", "######......", "######......", E, E, E, E, E, E, E]),
    # clipped at the right and bottom borders: band x 8..21 / y 7..31, interior x 10..19 / y 9..29
    ("right_bottom", [[9.0, 8.0, 20.0, 30.0]], [1],
     [E, E, E, E, E, E, E, "........####", "........####", "........##..", "........##..", "........##.."]),
    # degenerate x2 == x1: no interior, the whole band x 4..6 / y 1..10
    ("degenerate", [[5.0, 2.0, 5.9, 9.0]], [1],
     [E] + ["....###....."] * 10 + [E]),
    ("x2_below_x1", [[7.0, 2.0, 6.0, 9.0]], [1], [E] * 12),
    ("y2_below_y1", [[2.0, 7.0, 9.0, 6.9]], [1], [E] * 12),
    ("class_zero", [[3.7, 4.2, 8.9, 7.0]], [0], [E] * 12),
    ("not_finite", [[float("nan"), 4.2, 8.9, 7.0], [3.0, 4.0, float("inf"), 7.0]], [1, 1], [E] * 12),
]


@pytest.mark.parametrize("case", TRACED, ids=[c[0] for c in TRACED])
def test_draw_reference_on_hand_traced_cases(case):
    from dan_amd.utility import draw_toolbox
    _, boxes, classes, rows = case
    image = np.random.RandomState(5).randint(0, 200, (12, 12, 3)).astype(np.uint8)       # no pixel has the box colour's red 203
    out = draw_toolbox.draw_reference(image, classes, np.array(boxes, np.float32), thickness=2)
    mask = _mask(rows)
    assert np.array_equal((out == np.array(draw_toolbox.colors_tableau[1], np.uint8)).all(axis=2), mask)
    assert np.array_equal(out[~mask], image[~mask])                    # everything else is untouched
    assert draw_toolbox.colors_tableau[1] == (203, 71, 119)


def test_draw_reference_thickness_and_order():
    from dan_amd.utility import draw_toolbox
    image = np.zeros((12, 12, 3), np.uint8)
    one = draw_toolbox.draw_reference(image, [1], np.array([[4.0, 4.0, 8.0, 8.0]], np.float32), thickness=1)
    assert np.array_equal(np.argwhere(one[:, :, 0] == 203)[[0, -1]], [[4, 4], [8, 8]])             # t = 1: the outline itself, interior 5..7
    assert (one[5:8, 5:8] == 0).all() and int((one[:, :, 0] == 203).sum()) == 16
    boxes = np.array([[1.0, 1.0, 6.0, 6.0], [4.0, 3.0, 10.0, 9.0]], np.float32)
    assert np.array_equal(draw_toolbox.draw_reference(image, [1, 1], boxes), draw_toolbox.draw_reference(image, [1, 1], boxes[::-1]))
