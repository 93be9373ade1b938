"""The evaluation driver shared by eval_sfd / eval_pb / eval_dan / eval_dan_deform: `python -m dan_amd.eval_dan --data_dir WIDER_ROOT
--checkpoint_path M` does what the reference's `python eval_dan.py` does (eval_dan.py:299-466): restore the newest checkpoint, walk the
events of the subset, detect (origin, flip, multi-scale and - except for S3FD, whose script has none - the pyramid pass, merged by box
voting), write det_dir/<subset>/<event>/<name>.txt with the model's write_to_txt, and on every log_every_n_steps-th image of an event draw
the boxes with score > 0.2 on the image and write it to debug_dir/<name>.jpg.

Flags carry the reference's names and defaults (each script's tf.app.flags block; tests/golden/eval_flags.json).  Accepted and ignored:
data_format, num_classes, train_image_size and batch_size (the reference's graph takes one image of any size; they configure nothing
there either).  The port's own: --device, --precision, --batch_images (JPEGs read, decoded and detected as one group), --decode_entropy, --encode_entropy,
--encode_optimize (the debug images' encoder makes each image's own Huffman tables, as Pillow's optimize=True; off by default), --image_list (one `event/name` per line instead of wider_face_split/wider_face_<subset>.mat, which needs scipy), --gt_dir (the directory
of wider_face_<subset>.mat / wider_easy_<subset>.mat / wider_medium_<subset>.mat / wider_hard_<subset>.mat: the average precision is
computed on the device and printed), --debug_quality, --debug_labels (draw each box's score on a tab above it; off by default), --chips_dir (with --chips_size, --chips_margin and
--chips_threshold: every detection of score >= the threshold cropped and resized on the device by utility.face_chips' rule and written to
chips_dir/<event>/<name>_<row>.jpg through the debug images' encoder, one encode call per group; off by default, and then nothing changes;
--chips_filter {linear,area} and --chips_pad choose the antialiased downscale and the whole, black-padded square instead of the clipped one) and
--redact_dir (with --redact_mode {blur,mosaic,fill}, --redact_shape {rect,ellipse}, --redact_strength, --redact_margin and
--redact_threshold: EVERY image of the run with its detections of score >= the threshold made unrecognisable on the device by
utility.redact's rule and written to redact_dir/<event>/<name>.jpg through the debug images' encoder, one encode call per group; off by
default, and then nothing changes) and
--lfpn_upsample {bilinear,transposed} (eval_pb, eval_dan, eval_dan_deform; default bilinear): the graph of a checkpoint trained with
train_*'s flag of the same name.  transposed has no split-operand form: with --precision split the command exits with a message.
--backbone {vgg16,resnet50,resnet101,resnet152} (eval_dan; default vgg16) is train_dan's flag of the same name: batch norm runs on the
checkpoint's moving statistics.  It has no fp32 or split-operand kernel: a ResNet backbone runs with --precision act only (a message otherwise).

Per group: the files are read, decoded on the device (dataset.jpeg.JpegDecoder; a stream it refuses takes its Pillow fallback) and
detected (eval_dan.detect_image_list); ONE download brings (dets, num) to the host for the text files; the evaluator takes the device
tensors; the debug images of the group are drawn in one launch where the decoder left them (utility.draw_toolbox: rectangles, and with
--debug_labels the score labels by the module's own rule) and encoded in one batch (dataset.jpeg.JpegEncoder: byte for byte Pillow's JPEG
at --debug_quality).
--debug_dir "" writes no images and never touches the encoder."""
import argparse
import collections
import os
import sys

REFERENCE_FLAGS = collections.OrderedDict([
    # scaffold related configuration
    ("det_dir", "./sfd_det/"), ("debug_dir", "./sfd_debug/"), ("data_dir", "WIDER_ROOT"), ("subset", "val"), ("train_image_size", 640),
    ("num_classes", 2), ("log_every_n_steps", 10),
    # model related configuration
    ("batch_size", 1), ("data_format", "channels_last"),
    ("nms_threshold", 0.3), ("memory_limit", 577.0), ("max_per_image", 750), ("select_threshold", 0.01),
    # checkpoint related configuration
    ("checkpoint_path", "./sfd_logs"), ("model_scope", "sfd"),
])
MODEL_FLAGS = {       # what each script's flag block changes against eval_sfd.py's
    "sfd": {},
    "pb": dict(det_dir="./pd_det/", debug_dir="./pb_debug/", checkpoint_path="./pyramid_box_logs", model_scope="pyramid_box"),
    "dan": dict(det_dir="./dan_det/", debug_dir="./dan_debug/", checkpoint_path="./dan_logs/", model_scope="dan"),
    "dan_deform": dict(det_dir="./dan_det/", debug_dir="./dan_debug/", checkpoint_path="./dan_logs_deform/", model_scope="dan"),
}
IGNORED_FLAGS = ("data_format", "num_classes", "train_image_size", "batch_size")
_HELP = {
    "det_dir": "where the prediction files go: det_dir/<subset>/<event>/<name>.txt",
    "debug_dir": "where the drawn images go: debug_dir/<name>.jpg (\"\": none are written)",
    "data_dir": "the dataset root: WIDER_<subset>/images/<event>/<name>.jpg and wider_face_split/", "subset": "val or test",
    "log_every_n_steps": "every n-th image of an event is drawn and written to debug_dir",
    "nms_threshold": "overlap above which box voting merges detections", "memory_limit": "the scale ratio of get_shrink",
    "max_per_image": "detections kept per image", "select_threshold": "score a detection needs to be written",
    "checkpoint_path": "checkpoint prefix, or directory whose newest checkpoint is restored", "model_scope": "scope of the variables in it",
}
DEBUG_SCORE = 0.2            # eval_dan.py:456
PYRAMID = {"sfd": False, "pb": True, "dan": True, "dan_deform": True}       # eval_sfd.py:323-328 has no multi_scale_test_pyramid
MIN_HEIGHT = {"sfd": 10, "pb": 9, "dan": 10, "dan_deform": 10}              # write_to_txt's row filter (eval_pb.py:252)
LFPN_UPSAMPLE = ("bilinear", "transposed")                                  # --lfpn_upsample (net/pb_net.py LFPN_UPSAMPLE)
BACKBONES = ("vgg16", "resnet50", "resnet101", "resnet152")                 # --backbone (train_dan.BACKBONES)


def flag_defaults(model):
    d = collections.OrderedDict(REFERENCE_FLAGS)
    d.update(MODEL_FLAGS[model])
    return d


def build_parser(model):
    p = argparse.ArgumentParser(prog="python -m dan_amd.eval_%s" % model,
                                description="Evaluate %s on WIDER FACE: prediction files, debug images and (with --gt_dir) the AP, on one MI355X." % model)
    for name, default in flag_defaults(model).items():
        text = "accepted for the reference's command lines and ignored" if name in IGNORED_FLAGS else _HELP.get(name, "as the reference's flag")
        if name == "subset":
            p.add_argument("--subset", choices=("val", "test"), default=default, help=text + " (default %r)" % default)
        else:
            p.add_argument("--" + name, type=type(default), default=default, help=text + " (default %r)" % (default,))
    p.add_argument("--device", default="cuda:0", help="the GPU to evaluate on (default cuda:0)")
    p.add_argument("--precision", choices=("act", "fp32", "split"), default="act", help="eval_dan.Detector's precision (default act)")
    p.add_argument("--batch_images", type=int, default=8, help="images read, decoded and detected as one group (default 8)")
    p.add_argument("--decode_entropy", choices=("host", "device"), default="host", help="where the JPEG Huffman stage of the decoder runs (default host)")
    p.add_argument("--encode_entropy", choices=("host", "device"), default="host",
                   help="where the JPEG Huffman stage of the debug images' encoder runs (default host; the files are the same bytes)")
    p.add_argument("--encode_optimize", action="store_true",
                   help="debug images with Huffman tables of their own, as Pillow's save(optimize=True): the same pixels in smaller files (default off)")
    p.add_argument("--image_list", default=None, help="text file with one event/name per line, instead of wider_face_split/wider_face_<subset>.mat")
    p.add_argument("--gt_dir", default=None, help="directory of wider_face_<subset>.mat and wider_{easy,medium,hard}_<subset>.mat: compute and print the AP")
    p.add_argument("--debug_quality", type=int, default=75, help="JPEG quality of the debug images (default 75)")
    p.add_argument("--debug_labels", action="store_true",
                   help="draw each box's score ('%%.1f%%%%' of score * 100) in white on a filled tab above it (default: rectangles only)")
    p.add_argument("--chips_dir", default=None,
                   help="write every detection as a face chip to chips_dir/<event>/<name>_<row>.jpg at --debug_quality (default: none are made)")
    p.add_argument("--chips_size", type=int, default=112, help="side of a face chip in pixels, 1 .. 1024 (default 112)")
    p.add_argument("--chips_margin", type=float, default=0.0,
                   help="fraction of the box side added on each side before the crop is squared and clipped to the image, 0 .. 4 (default 0)")
    p.add_argument("--chips_threshold", type=float, default=None, help="score a detection needs to become a chip (default: --select_threshold)")
    p.add_argument("--chips_filter", choices=("linear", "area"), default="linear",
                   help="how a chip is resized: linear (OpenCV's INTER_LINEAR, default) or area (antialiased: a box filter where the crop shrinks)")
    p.add_argument("--chips_pad", action="store_true",
                   help="keep the squared crop whole and fill what leaves the image with black, instead of clipping it to the image (default off)")
    p.add_argument("--redact_dir", default=None,
                   help="write every image with its detections redacted to redact_dir/<event>/<name>.jpg at --debug_quality (default: none are made)")
    p.add_argument("--redact_mode", choices=("blur", "mosaic", "fill"), default="blur",
                   help="what replaces a face: a box blur scaled to it (default), a mosaic of cell means, or black")
    p.add_argument("--redact_shape", choices=("rect", "ellipse"), default="rect", help="the box itself (default) or the ellipse inscribed in it")
    p.add_argument("--redact_strength", type=float, default=0.125,
                   help="blur radius / mosaic cell side as a fraction of the box's longer side, 0.001 .. 1 (default 0.125)")
    p.add_argument("--redact_margin", type=float, default=0.0, help="fraction of the box side added on each side, 0 .. 4 (default 0)")
    p.add_argument("--redact_threshold", type=float, default=None, help="score a detection needs to be redacted (default: --select_threshold)")
    if model != "sfd":                                                      # (S3FD has no LFPN)
        p.add_argument("--lfpn_upsample", choices=LFPN_UPSAMPLE, default="bilinear",
                       help="the LFPN of the checkpoint's graph: bilinear resize (default) or the learnable 4x4 stride-2 transposed convolution "
                            "(train_*'s --lfpn_upsample transposed); transposed does not run with --precision split")
    if model == "dan":                                                      # (the reference has no deformable ResNet backbone)
        p.add_argument("--backbone", choices=BACKBONES, default="vgg16",
                       help="the backbone of the checkpoint's graph: vgg16 (default) or a ResNet with batch norm (train_dan's --backbone); "
                            "a ResNet runs with --precision act only")
    return p


# ------------------------------------------------------------------------------------------------------------ the file list
def read_image_list(path):
    """One `event/name` per line (a trailing .jpg is dropped, blank lines and # comments skipped) -> [(event, [name, ...])] in the order of
    the events' first lines."""
    events = collections.OrderedDict()
    with open(path) as f:
        for line in f:
            line = line.strip()
            if not line or line.startswith("#"):
                continue
            if line.lower().endswith(".jpg"):
                line = line[:-4]
            event, sep, name = line.rpartition("/")
            if not sep or not event or not name:
                raise ValueError("%s: %r is not event/name" % (path, line))
            events.setdefault(event, []).append(name)
    return list(events.items())


def read_mat_list(path):
    """event_list / file_list of wider_face_<subset>.mat (eval_dan.py:416-434) -> [(event, [name, ...])]."""
    import numpy as np
    import scipy.io                                              # only here: the command runs from --image_list without scipy

    def cells(a):
        return list(np.asarray(a, dtype=object).reshape(-1))

    def text(a):
        return str(np.asarray(a).reshape(-1)[0])

    mat = scipy.io.loadmat(path)
    files = cells(mat["file_list"])
    return [(text(event), [text(f) for f in cells(files[e])]) for e, event in enumerate(cells(mat["event_list"]))]


def file_list(args):
    if args.image_list:
        return read_image_list(args.image_list)
    return read_mat_list(os.path.join(args.data_dir, "wider_face_split", "wider_face_%s.mat" % args.subset))


def ground_truth(args):
    from .wider_eval import WiderGroundTruth
    d, s = args.gt_dir, args.subset
    return WiderGroundTruth.from_mat(os.path.join(d, "wider_face_%s.mat" % s), os.path.join(d, "wider_easy_%s.mat" % s),
                                     os.path.join(d, "wider_medium_%s.mat" % s), os.path.join(d, "wider_hard_%s.mat" % s))


# ------------------------------------------------------------------------------------------------------------ the models
def build_detector(model, device, precision, seed=20180817, lfpn_upsample="bilinear", backbone="vgg16"):
    """eval_dan.Detector around the model's inference graph with its script's anchors.  The variables are created here, by one forward
    of a 64 x 64 image (their shapes do not depend on the image size), so that a checkpoint finds them: the store makes a variable when a
    layer first asks for it."""
    import torch
    from . import eval_dan
    from .train_sfd import AnchorConfig
    if model == "sfd":
        from .train_sfd import SFDModel
        net = eval_dan.Detector(SFDModel(device=device, seed=seed), lambda h, w, d: AnchorConfig(h, w, d), precision)
    elif model == "pb":
        from .train_pb import PBModel
        net = eval_dan.Detector(PBModel(device=device, seed=seed, lfpn_upsample=lfpn_upsample), lambda h, w, d: AnchorConfig(h, w, d), precision)     # ratios (1.,): eval_pb.py:311
    else:
        from .train_dan import DANModel, dan_anchor_config
        net = eval_dan.Detector(DANModel(device=device, seed=seed, deform=(model == "dan_deform"), lfpn_upsample=lfpn_upsample, backbone=backbone), dan_anchor_config,
                                precision)
    with torch.no_grad():
        net.model.forward(torch.zeros((1, 64, 64, 3), dtype=torch.uint8, device=device))
    return net


def written_rows(det, select_threshold, min_height):
    """What write_to_txt writes of fp32 rows (xmin, ymin, xmax, ymax, score), as float64 [n,5] rows (x, y, w, h, score): the evaluator's
    input when the model's filter is not the one danhip_wider_quantize applies on the device."""
    import numpy as np
    xmin, ymin, xmax, ymax, sc = (det[:, i] for i in range(5))
    bh, bw = ymax - ymin + 1, xmax - xmin + 1
    valid = np.logical_and(np.logical_and(np.ceil(bh) >= min_height, bw > 1), sc > select_threshold)
    rows = np.stack([np.floor(xmin), np.floor(ymin), np.ceil(bw), np.ceil(bh), np.asarray(["%.3f" % v for v in sc], dtype=np.float64)], axis=1)
    return rows[valid].astype(np.float64).reshape(-1, 5)


# ------------------------------------------------------------------------------------------------------------ main
def main(argv=None, model="sfd", gt=None, out=None):
    """gt: a wider_eval.WiderGroundTruth to score against (instead of --gt_dir); out: where the progress and AP lines go (sys.stdout).
    -> {"images": n, "debug": [paths], "chips": [paths], "redacted": [paths], "ap": {subset: AP} or None, "decoder": stats, "encoder": stats or None}."""
    args = build_parser(model).parse_args(argv)
    out = sys.stdout if out is None else out
    if args.batch_images < 1:
        raise SystemExit("--batch_images %d: at least 1" % args.batch_images)
    if not 1 <= args.debug_quality <= 100:
        raise SystemExit("--debug_quality %d: 1 .. 100" % args.debug_quality)
    if args.chips_dir:
        from .utility import face_chips                           # (importing it does not touch the device)
        try:
            face_chips.check_size(args.chips_size)
            chips_pm = face_chips.margin_per_mille(args.chips_margin)
        except ValueError as e:
            raise SystemExit("--chips_size / --chips_margin: %s" % e)
        chips_threshold = args.select_threshold if args.chips_threshold is None else args.chips_threshold
        # (--chips_filter is one of argparse's choices; either new flag takes danhip_face_chips_u8_ex, whose rule has a side cap)
        chips_cap = face_chips.MAX_SIDE if args.chips_filter != "linear" or args.chips_pad else None
    if args.redact_dir:
        from .utility import redact                               # (importing it does not touch the device)
        try:
            redact.strength_per_mille(args.redact_strength)
            redact.margin_per_mille(args.redact_margin)
            redact_threshold = redact.check_threshold(args.select_threshold if args.redact_threshold is None else args.redact_threshold)
        except ValueError as e:
            raise SystemExit("--redact_strength / --redact_margin / --redact_threshold: %s" % e)
    lfpn_upsample = getattr(args, "lfpn_upsample", "bilinear")
    if lfpn_upsample == "transposed" and args.precision == "split":
        raise SystemExit("--lfpn_upsample transposed has no split-operand form: use --precision act or fp32")
    backbone = getattr(args, "backbone", "vgg16")
    if backbone != "vgg16" and args.precision != "act":
        raise SystemExit("--backbone %s runs with --precision act only: batch norm has no fp32 or split-operand kernel" % backbone)
    import numpy as np
    import torch
    from . import eval_dan
    from .dataset.jpeg import JpegDecoder, JpegEncoder
    from .utility import checkpoint, draw_toolbox
    from .wider_eval import WiderEvaluator
    device = torch.device(args.device)
    torch.cuda.set_device(device)
    events = file_list(args)
    if gt is None and args.gt_dir:
        gt = ground_truth(args)

    net = build_detector(model, device, args.precision, lfpn_upsample=lfpn_upsample, backbone=backbone)
    path = args.checkpoint_path
    if os.path.isdir(path):
        path = checkpoint.latest_checkpoint(path)
    if not path or not os.path.exists(path + ".index"):
        raise SystemExit("no checkpoint at %s" % args.checkpoint_path)
    names = checkpoint.restore_checkpoint(net.model.vs, path, args.model_scope, verify=True)
    if not names:
        raise SystemExit("checkpoint %s holds no variable of scope %s" % (path, args.model_scope))
    print("restored %s: %d variables" % (path, len(names)), file=out, flush=True)

    decoder = JpegDecoder(device, entropy=args.decode_entropy)
    encoder = JpegEncoder(quality=args.debug_quality, entropy=args.encode_entropy, optimize=args.encode_optimize) if args.debug_dir else None
    if args.debug_dir:
        os.makedirs(args.debug_dir, exist_ok=True)
    chip_encoder = JpegEncoder(quality=args.debug_quality, entropy=args.encode_entropy, optimize=args.encode_optimize) if args.chips_dir else None
    redact_encoder = JpegEncoder(quality=args.debug_quality, entropy=args.encode_entropy, optimize=args.encode_optimize) if args.redact_dir else None
    min_height = MIN_HEIGHT[model]
    on_device = min_height == 10 and args.select_threshold == eval_dan.SELECT_THRESHOLD       # the filter danhip_wider_quantize restates
    evaluator = None
    if gt is not None:
        evaluator = WiderEvaluator(gt, quantize=on_device, max_per_image=args.max_per_image, device=device)
    image_root = os.path.join(args.data_dir, "WIDER_val" if args.subset == "val" else "WIDER_test", "images")
    save_root = os.path.join(args.det_dir, args.subset)
    every = max(args.log_every_n_steps, 1)
    total, debug_paths, chip_paths, redact_paths = 0, [], [], []
    for index, (event, files) in enumerate(events):
        os.makedirs(os.path.join(save_root, event), exist_ok=True)
        for start in range(0, len(files), args.batch_images):
            group = files[start:start + args.batch_images]
            datas = []
            for name in group:
                with open(os.path.join(image_root, event, name + ".jpg"), "rb") as f:
                    datas.append(f.read())
            images = decoder.decode_batch(datas)
            dets, num = eval_dan.detect_image_list(net, images, PYRAMID[model], args.nms_threshold, args.max_per_image, args.memory_limit)
            B = len(group)
            host = torch.cat((dets.reshape(B, -1), num.reshape(B, 1).to(torch.float32)), dim=1).cpu()      # the one download: counts <= 750 are exact
            counts = [int(v) for v in host[:, -1].tolist()]
            rows = host[:, :-1].reshape(B, -1, 5).numpy()
            for b, name in enumerate(group):
                with open(os.path.join(save_root, event, name + ".txt"), "w") as f:
                    eval_dan.write_to_txt(f, rows[b, :counts[b]], event, name, args.select_threshold, min_height=min_height)
            if evaluator is not None:
                index_of = [gt.index_of(event + "/" + name) for name in group]
                if on_device:
                    evaluator.add(index_of, dets, num)
                else:
                    for b, i in enumerate(index_of):
                        evaluator.add_rows(i, torch.from_numpy(written_rows(rows[b, :counts[b]], args.select_threshold, min_height)))
            if redact_encoder is not None:                       # before the debug images: those are drawn in place
                pictures, _ = redact.apply(images, dets, num, mode=args.redact_mode, shape=args.redact_shape, strength=args.redact_strength,
                                           margin=args.redact_margin, score_threshold=redact_threshold)
                os.makedirs(os.path.join(args.redact_dir, event), exist_ok=True)
                for name, data in zip(group, redact_encoder.encode_batch(pictures)):
                    redact_paths.append(os.path.join(args.redact_dir, event, name + ".jpg"))
                    with open(redact_paths[-1], "wb") as f:
                        f.write(data)
            drawn = [b for b in range(B) if (start + b) % every == 0] if encoder is not None else []
            if drawn:
                boxes = [dets[b, :counts[b], :4] for b in drawn]
                classes = [(dets[b, :counts[b], 4] > DEBUG_SCORE).to(torch.int32) for b in drawn]
                pictures = draw_toolbox.bboxes_draw_on_img_list([images[b].contiguous() for b in drawn], classes, [dets[b, :counts[b], 4] for b in drawn],
                                                                boxes, thickness=2, labels=args.debug_labels)
                for b, data in zip(drawn, encoder.encode_batch(pictures)):
                    debug_paths.append(os.path.join(args.debug_dir, group[b] + ".jpg"))
                    with open(debug_paths[-1], "wb") as f:
                        f.write(data)
            if chip_encoder is not None:
                # the rows that give a chip, from the rows already on the host (the rule is integers only: host and device agree), so the
                # chip buffer is sized to them and the files are named without a second download
                thr = np.float32(chips_threshold)
                owners = [(b, r) for b in range(B) for r in range(counts[b]) if not rows[b, r, 4] < thr and
                          face_chips.rule(rows[b, r], int(images[b].shape[0]), int(images[b].shape[1]), chips_pm, True, pad=args.chips_pad,
                                          cap=chips_cap) is not None]
                if owners:
                    chips = face_chips.extract(images, dets, num, size=args.chips_size, margin=args.chips_margin, square=True,
                                               score_threshold=chips_threshold, max_chips=len(owners), filter=args.chips_filter,
                                               pad=args.chips_pad).chips
                    os.makedirs(os.path.join(args.chips_dir, event), exist_ok=True)
                    for (b, r), data in zip(owners, chip_encoder.encode_batch(list(chips))):
                        chip_paths.append(os.path.join(args.chips_dir, event, "%s_%d.jpg" % (group[b], r)))
                        with open(chip_paths[-1], "wb") as f:
                            f.write(data)
            total += B
            out.write("\r>> Predicting event:%d/%d num:%d/%d" % (index + 1, len(events), start + B, len(files)))
            out.flush()
        out.write("\n")
        out.flush()
    ap = None
    if evaluator is not None:
        res = evaluator.result()
        ap = collections.OrderedDict((s, res[s]) for s in gt.subsets)
        for s, v in ap.items():
            print("%s AP: %.6f" % (s, v), file=out, flush=True)
    return {"images": total, "debug": debug_paths, "chips": chip_paths, "redacted": redact_paths, "ap": ap, "decoder": decoder.stats, "encoder": None if encoder is None else encoder.stats}
