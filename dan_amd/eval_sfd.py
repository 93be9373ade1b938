"""eval_sfd.py's test-time pipeline (:60-196, :323-330): the same helpers as eval_dan.py without the pyramid pass."""
from .eval_dan import (Detector, bbox_vote, bbox_vote_batch, detect_face, flip_test, get_shrink, multi_scale_test,  # noqa: F401
                       resize_image, write_to_txt)
from .eval_dan import detect_image as _detect_image


def detect_image(net, image):
    """eval_sfd.py:323-328: origin + flip + multi-scale, merged by box voting."""
    return _detect_image(net, image, pyramid=False)


def detect_images(net, images):
    """The same passes for B images of one size, batched (eval_dan.detect_images): (dets [B, 750, 5], num [B]) on the device."""
    from .eval_dan import detect_images as _detect_images
    return _detect_images(net, images, pyramid=False)


def detect_image_list(net, images):
    """The same passes for images of different sizes (eval_dan.detect_image_list): (dets [B, 750, 5], num [B]) on the device."""
    from .eval_dan import detect_image_list as _detect_image_list
    return _detect_image_list(net, images, pyramid=False)


def detect_encoded(net, datas, decoder):
    """JPEG byte strings -> detections (eval_dan.detect_encoded) without the pyramid pass."""
    from .eval_dan import detect_encoded as _detect_encoded
    return _detect_encoded(net, datas, decoder, pyramid=False)


def main(argv=None, **kw):
    """`python -m dan_amd.eval_sfd --data_dir WIDER_ROOT --checkpoint_path M`: the reference's `python eval_sfd.py` (dan_amd/eval_cli.py)."""
    from .eval_cli import main as run
    return run(argv, model="sfd", **kw)


if __name__ == "__main__":
    main()
