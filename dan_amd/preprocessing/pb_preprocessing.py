"""Training input pipeline of the reference's preprocessing/pb_preprocessing.py on the GPU (what train_pb.py feeds PyramidBox).

In the reference this file is dan_preprocessing.py under other names: a textual diff of the two shows `sfd_random_sample_patch_wrapper` /
`sfd_random_sample` in place of `dan_random_sample_patch_wrapper` / `dan_random_sample` (pb_preprocessing.py:410-493, :623-635, :702), the
name_scope strings (:689, :744) and one deleted comment, nothing else.  So this module is that surface over the functions of
dan_preprocessing.py - no body is restated - and everything said there holds here: the geometric functions decide a crop window and the
boxes on the host, one device pass produces the network input.

Order of the draws, per image, from one `Draws` (the order pb_preprocessing.py reaches its random ops; identical to the DAN module's):
  1. randint(0, 4): the colour ordering; 2. the four colour draws in the order that ordering applies its ops;
  3. uniform(0, 1) < 0.5 chooses sfd_random_sample, else data_anchor_sampling (:702);
  4a. sfd_random_sample: uniform(0.3, 1) x 4, choice(5), per attempt randint x, randint y (at most 25), then - only when all were rejected -
      randint(0, number of boxes);
  4b. data_anchor_sampling: randint(0, number of boxes) (the face), randint(0, anchor_ind) (the target scale), uniform (the final scale),
      randint x, randint y (the patch position);
  5. uniform(0, 1) < 0.5: the flip, of the resized image.
preprocess_batch_for_train takes these for image 0, then image 1, ... from the one `Draws` it is given."""
from .dan_preprocessing import (Draws, augment_batch, augment_image, data_anchor_sampling, distort_color, preprocess_batch_for_train,  # noqa: F401
                                preprocess_for_train, pyramid_box_random_sample_patch_wrapper, random_flip_left_right)
from .dan_preprocessing import dan_random_sample as sfd_random_sample  # noqa: F401
from .dan_preprocessing import dan_random_sample_patch_wrapper as sfd_random_sample_patch_wrapper  # noqa: F401
