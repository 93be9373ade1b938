"""eval_dan_deform.py's test-time pipeline: eval_dan.py's, line for line, around the deformable backbone (train_dan.DANModel(deform=True));
the script differs from eval_dan.py in the backbone import and in its default checkpoint_path, './dan_logs_deform/'."""
from .eval_dan import (Detector, bbox_vote, bbox_vote_batch, detect_encoded, detect_face, detect_image, detect_image_list,  # noqa: F401
                       detect_images, flip_test, get_shrink, multi_scale_test, multi_scale_test_pyramid, resize_image, write_to_txt)


def main(argv=None, **kw):
    """`python -m dan_amd.eval_dan_deform --data_dir WIDER_ROOT --checkpoint_path M`: the reference's `python eval_dan_deform.py`."""
    from .eval_cli import main as run
    return run(argv, model="dan_deform", **kw)


if __name__ == "__main__":
    main()
