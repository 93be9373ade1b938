"""Training / evaluation input pipeline of the reference's preprocessing/sfd_preprocessing.py on the GPU (what train_sfd.py feeds S3FD).

Same function names and argument order as the reference (distort_color, sfd_random_sample_patch_wrapper, random_flip_left_right,
preprocess_for_train, preprocess_for_eval, preprocess_image), re-cut for the device exactly as dan_preprocessing.py is: the host decides the
colour chain, the crop WINDOW and the boxes; one device pass (dan_preprocessing.augment_batch -> danhip_augment_preprocess_batch) produces the
network input.  There is NO data-anchor-sampling branch, no draw for one and no `anchor_scales` argument (sfd_preprocessing.py:495).

Compared with dan_preprocessing.py, line by line:
  * distort_color (:98-150) and random_flip_left_right (:481-493) have the bodies of the DAN module's (:98-150, :609-621): the DAN functions
    are called.
  * sfd_random_sample_patch_wrapper (:353-436) and dan_random_sample_patch_wrapper (dan_preprocessing.py:410-493) differ in the function
    name and the name_scope string only (a textual diff of the two ranges shows nothing else): strict inequalities in the 25-attempt loop
    (:394-395), non-strict ones and the clip to [0, size - 1] in sample_around_bbox (:366-370), tf.to_int32 truncation of the window
    (:373, :405), the same clipping of the boxes (:426-434).  The DAN function is called.
  * preprocess_for_train (:495-552) DOES differ from the DAN one (dan_preprocessing.py:677-733), in where the flip sits:
      - :522 flips the cropped window BEFORE :531 resizes it; DAN resizes (:707) and flips the resized image (:714).  With the legacy
        bilinear resize (source = destination * in / out, no half-pixel centre) the two are different images: FLIP_WINDOW in the item
        (flip = 2 of danhip_augment_item) mirrors the window's columns and then resizes.
      - the boxes are mirrored about the WINDOW's width (:490-491 on random_sample_image, float_width - 1 - x) and rescaled to out_shape
        afterwards (:526-530); DAN rescales first and mirrors about out_shape[1].
    Both are implemented here as the reference's lines state them.

Order of the draws (this project's contract; the reference's TF random ops define no reproducible stream), per image, from one `Draws`:
  1. randint(0, 4): the colour ordering (apply_with_random_selector, :515-517);
  2. the four colour draws in the order that ordering applies its ops (brightness uniform(-32/255, 32/255), saturation / contrast
     uniform(0.5, 1.5), hue uniform(-0.2, 0.2));
  3. the patch wrapper: uniform(0.3, 1) x 4 (patch_a .. patch_d, :411-414), choice(5) (:417), then per attempt randint x, randint y
     (:389-390) for at most 25 attempts, then - only when every attempt was rejected - randint(0, number of boxes) (:364);
  4. uniform(0, 1) < 0.5: the flip (:485-486).
preprocess_batch_for_train takes these for image 0, then image 1, ... from the one `Draws` it is given.

preprocess_for_eval (:554-580): with out_shape=None (what the reference's evaluation scripts pass) it is mean subtraction + BGR of the
uint8 image (danhip_preprocess_u8).  With an out_shape the reference resizes the FLOAT image (legacy bilinear, no uint8 step after it)
before the means; the library has no kernel of that form (danhip_resize_u8_linear is cv2's 8-bit resize, danhip_resize_bilinear_add_fwd
adds feature maps), so that case raises ValueError."""
import numpy as np

from . import dan_preprocessing as _dan
from .dan_preprocessing import Draws, F, FLIP_NONE, FLIP_WINDOW, distort_color, random_flip_left_right  # noqa: F401  (the module's surface)


def sfd_random_sample_patch_wrapper(height, width, bboxes, draws):
    """sfd_preprocessing.py:353-436 -> ((y, x, h, w), boxes in window coordinates); the body of dan_random_sample_patch_wrapper."""
    return _dan.dan_random_sample_patch_wrapper(height, width, bboxes, draws)


def draw_for_train(height, width, bboxes, out_shape, draws):
    """The draws and the box arithmetic of preprocess_for_train (:515-551) -> (ops, window, flip flag, boxes after the small-box filter)."""
    bboxes = np.asarray(bboxes, F).reshape(-1, 4)
    ops = distort_color(draws.randint(0, 4), draws, fast_mode=False)                  # :515-517
    window, boxes = sfd_random_sample_patch_wrapper(height, width, bboxes, draws)    # :519
    flip, boxes = random_flip_left_right(boxes, window[3], draws)                     # :522, about the window's width
    th, tw, fh, fw = F(out_shape[0]), F(out_shape[1]), F(window[2]), F(window[3])     # :524-530
    boxes = np.stack([boxes[:, 0] * th / fh, boxes[:, 1] * tw / fw, boxes[:, 2] * th / fh, boxes[:, 3] * tw / fw], -1).astype(F)
    keep = ((boxes[:, 2] - boxes[:, 0]) > F(6.)) & ((boxes[:, 3] - boxes[:, 1]) > F(3.))   # :544-551
    return ops, window, bool(flip), boxes[keep]


def _to_numpy(bboxes):
    return bboxes.detach().cpu().numpy() if hasattr(bboxes, "detach") else bboxes


def _check_format(data_format, output_rgb):
    if data_format != "channels_last" or output_rgb:
        raise ValueError("the MI355X build feeds NHWC BGR (the reference's training scripts pass output_rgb=False)")


def preprocess_for_train(image, bboxes, out_shape, data_format="channels_last", scope=None, output_rgb=False, draws=None):
    """sfd_preprocessing.py:495-552.  image: uint8 [H,W,3] RGB device tensor; bboxes: float32 [n,4] (ymin,xmin,ymax,xmax) in pixels.
    -> (network input [out_h,out_w,8] 16-bit BGR mean-subtracted, boxes float32 [k,4] numpy in output pixels; small boxes dropped)."""
    _check_format(data_format, output_rgb)
    ops, window, flip, boxes = draw_for_train(int(image.shape[0]), int(image.shape[1]), _to_numpy(bboxes), out_shape, draws or Draws())
    out = _dan.augment_batch([image], [(ops, window, FLIP_WINDOW if flip else FLIP_NONE)], out_shape)[0]
    out._real_channels = 3
    return out, boxes


def preprocess_batch_for_train(images, bboxes_list, out_shape, data_format="channels_last", scope=None, output_rgb=False, draws=None):
    """preprocess_for_train for a decoded group -> (network input [K,out_h,out_w,8], list of K box arrays, list of the K kept indices): the
    draws of image 0, then image 1, ... from one `draws`; images whose boxes are all gone are dropped before the one device pass."""
    _check_format(data_format, output_rgb)

    def host_half(image, bboxes, d):
        ops, window, flip, boxes = draw_for_train(int(image.shape[0]), int(image.shape[1]), _to_numpy(bboxes), out_shape, d)
        return ops, window, FLIP_WINDOW if flip else FLIP_NONE, boxes

    return _dan.batch_for_train(images, bboxes_list, out_shape, host_half, draws)


def preprocess_for_eval(image, out_shape, data_format="channels_last", scope=None, output_rgb=False):
    """sfd_preprocessing.py:554-580 with out_shape=None: uint8 [H,W,3] RGB device tensor -> (network input [H,W,8], (H, W))."""
    _check_format(data_format, output_rgb)
    if out_shape is not None:
        raise ValueError("preprocess_for_eval resizes the float image before the means when out_shape is given; the library has no legacy "
                         "bilinear resize of that form - pass out_shape=None (as the reference's evaluation scripts do)")
    from .. import ops
    out = ops.preprocess_u8(image.unsqueeze(0))[0]
    out._real_channels = 3
    return out, (int(image.shape[0]), int(image.shape[1]))


def preprocess_image(image, bboxes, out_shape, is_training=False, data_format="channels_last", output_rgb=False, draws=None):
    """sfd_preprocessing.py:582-598."""
    if is_training:
        return preprocess_for_train(image, bboxes, out_shape, data_format=data_format, output_rgb=output_rgb, draws=draws)
    return preprocess_for_eval(image, out_shape, data_format=data_format, output_rgb=output_rgb)
