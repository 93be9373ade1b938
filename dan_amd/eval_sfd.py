"""eval_sfd.py's test-time pipeline (:60-196, :323-330): the same helpers as eval_dan.py without the pyramid pass."""
from .eval_dan import (MAX_PER_IMAGE, MEMORY_LIMIT, NMS_THRESHOLD, Detector, bbox_vote, bbox_vote_batch, detect_face, flip_test,  # noqa: F401
                       get_shrink, multi_scale_test, resize_image, write_to_txt, detect_encoded as _detect_encoded,
                       detect_image as _detect_image, detect_image_list as _detect_image_list, detect_images as _detect_images)


def detect_image(net, image, nms_threshold=NMS_THRESHOLD, max_per_image=MAX_PER_IMAGE, memory_limit=MEMORY_LIMIT):
    """eval_sfd.py:323-328: origin + flip + multi-scale, merged by box voting."""
    return _detect_image(net, image, False, nms_threshold, max_per_image, memory_limit)


def detect_images(net, images, nms_threshold=NMS_THRESHOLD, max_per_image=MAX_PER_IMAGE, memory_limit=MEMORY_LIMIT):
    """The same passes for B images of one size, batched (eval_dan.detect_images): (dets [B, max_per_image, 5], num [B]) on the device."""
    return _detect_images(net, images, False, nms_threshold, max_per_image, memory_limit)


def detect_image_list(net, images, nms_threshold=NMS_THRESHOLD, max_per_image=MAX_PER_IMAGE, memory_limit=MEMORY_LIMIT):
    """The same passes for images of different sizes (eval_dan.detect_image_list): (dets [B, max_per_image, 5], num [B]) on the device."""
    return _detect_image_list(net, images, False, nms_threshold, max_per_image, memory_limit)


def detect_encoded(net, datas, decoder, nms_threshold=NMS_THRESHOLD, max_per_image=MAX_PER_IMAGE, memory_limit=MEMORY_LIMIT):
    """JPEG byte strings -> detections (eval_dan.detect_encoded) without the pyramid pass."""
    return _detect_encoded(net, datas, decoder, False, nms_threshold, max_per_image, memory_limit)


def main(argv=None, **kw):
    """`python -m dan_amd.eval_sfd --data_dir WIDER_ROOT --checkpoint_path M`: the reference's `python eval_sfd.py` (dan_amd/eval_cli.py)."""
    from .eval_cli import main as run
    return run(argv, model="sfd", **kw)


if __name__ == "__main__":
    main()
