"""eval_pb.py's test-time pipeline: the helpers of eval_dan.py (the pyramid pass included, eval_pb.py's main loop runs it) around the
PyramidBox inference graph - anchor ratios (1.,), the context prediction module in front of the face head (train_pb.PBModel.predict) - and
the one line of the script that differs: write_to_txt keeps rows whose ceil(height) is >= 9, not >= 10 (eval_pb.py:252).
The port's own flag --lfpn_upsample {bilinear,transposed} (default bilinear) selects the LFPN of the checkpoint's graph (dan_amd/eval_cli.py)."""
from .eval_dan import (Detector, bbox_vote, bbox_vote_batch, detect_encoded, detect_face, detect_image, detect_image_list,  # noqa: F401
                       detect_images, flip_test, get_shrink, multi_scale_test, multi_scale_test_pyramid, resize_image, SELECT_THRESHOLD)
from .eval_dan import write_to_txt as _write_to_txt

MIN_HEIGHT = 9               # eval_pb.py:252


def write_to_txt(f, det, event, im_name, select_threshold=SELECT_THRESHOLD):
    """eval_pb.py:243-261: eval_dan.write_to_txt with the row filter ceil(height) >= 9."""
    return _write_to_txt(f, det, event, im_name, select_threshold, min_height=MIN_HEIGHT)


def main(argv=None, **kw):
    """`python -m dan_amd.eval_pb --data_dir WIDER_ROOT --checkpoint_path M`: the reference's `python eval_pb.py` (dan_amd/eval_cli.py)."""
    from .eval_cli import main as run
    return run(argv, model="pb", **kw)


if __name__ == "__main__":
    main()
