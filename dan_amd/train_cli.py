"""The training driver shared by train_sfd / train_pb / train_dan / train_dan_deform: `python -m dan_amd.train_sfd --data_dir D --model_dir M`
does what the reference's `python train_sfd.py --data_dir D --model_dir M` does (train_*.py `main`, the Estimator's train loop): resume from
model_dir or warm-start from checkpoint_path, read the TFRecords through slim_get_batch (device JPEG decode, one augmentation pass per
decoded group, one anchor-encoding call per batch), step until max_number_of_steps, log the reference's tensors_to_log every
log_every_n_steps and keep the newest five `model.ckpt-<step>` checkpoints.

Flags carry the reference's names and defaults (each script's tf.app.flags block; tests/golden/train_flags.json).  Accepted and ignored, since
they configure TensorFlow's input threads, session and device placement: num_readers, num_preprocessing_threads, num_cpu_threads,
gpu_memory_fraction, data_format, multi_gpu (and save_summary_steps / save_checkpoints_secs, which the reference itself leaves unused or
feeds to summaries this port does not write).  Three flags are this port's own: --device, --deterministic, --decode_entropy; a fourth,
--no_prefetch, exists for measuring the loader thread against the plain generator (profiles/r15/train_driver.md); a fifth,
--lfpn_upsample {bilinear,transposed} (train_pb, train_dan, train_dan_deform; default bilinear: the reference's graph), makes the LFPN merge
through a learnable 4x4 / stride-2 transposed convolution (net/pb_net.py build_lfpn) - a checkpoint written without it resumes or warm-starts
with the new variables at their initialiser; a sixth, --backbone {vgg16,resnet50,resnet101,resnet152} (train_dan; default vgg16), trains DAN on
the reference's ResNet + batch-norm backbone (net/resnet_danet.py): seeded initialisers or a resume from model_dir - a warm start from
--checkpoint_path and --deterministic are refused with a message before the device is touched.  Checkpoints are written
with a CRC-32C on every tensor (checksums="device": packed and checksummed on the GPU, profiles/r16/checkpoint_crc.md) and every tensor CRC
is checked on resume and on a warm start before a variable is written; --no_checkpoint_checksums turns both off.

Out of scope: more than one rank (bench.py --gpus N is the multi-rank path; WORLD_SIZE > 1 is refused), average precision during training,
and the position of the input stream across a resume (the reference restarts its queue as well)."""
import argparse
import collections
import os
import queue
import threading

REFERENCE_FLAGS = collections.OrderedDict([
    # hardware related configuration
    ("num_readers", 12), ("num_preprocessing_threads", 36), ("num_cpu_threads", 0), ("gpu_memory_fraction", 1.),
    # scaffold related configuration
    ("data_dir", "./dataset/tfrecords"), ("num_classes", 2), ("model_dir", "./sfd_logs/"), ("log_every_n_steps", 10),
    ("save_summary_steps", 500), ("save_checkpoints_secs", 7200), ("save_checkpoints_steps", 10000),
    # model related configuration
    ("train_image_size", 640), ("train_epochs", None), ("max_number_of_steps", 120000), ("batch_size", 32), ("data_format", "channels_first"),
    ("negative_ratio", 3.), ("match_threshold", 0.4), ("neg_threshold", 0.4),
    # optimizer related configuration
    ("tf_random_seed", 20180817), ("weight_decay", 0.0005), ("momentum", 0.9), ("learning_rate", 1e-3), ("end_learning_rate", 0.000001),
    ("decay_boundaries", "1000, 80000, 100000"), ("lr_decay_factors", "0.1, 1, 0.1, 0.01"),
    # checkpoint related configuration
    ("checkpoint_path", "./model"), ("checkpoint_model_scope", "vgg_16"), ("model_scope", "sfd"),
    ("checkpoint_exclude_scopes", "sfd/multibox_head, sfd/additional_layers, sfd/l2_norm_layer_3, sfd/l2_norm_layer_4, sfd/l2_norm_layer_5"),
    ("ignore_missing_vars", True), ("multi_gpu", True),
])
_INT_FLAGS = ("num_readers", "num_preprocessing_threads", "num_cpu_threads", "num_classes", "log_every_n_steps", "save_summary_steps",
              "save_checkpoints_secs", "save_checkpoints_steps", "train_image_size", "train_epochs", "max_number_of_steps", "batch_size",
              "tf_random_seed")
IGNORED_FLAGS = ("num_readers", "num_preprocessing_threads", "num_cpu_threads", "gpu_memory_fraction", "data_format", "multi_gpu",
                 "save_summary_steps", "save_checkpoints_secs")
_HELP = {
    "data_dir": "directory of the TFRecord files (train-*)", "model_dir": "where checkpoints and train.log go; a checkpoint found here is resumed",
    "log_every_n_steps": "steps between log lines (the host reads device scalars only then)",
    "save_checkpoints_steps": "steps between checkpoints (one more at the end; the newest 5 are kept)",
    "train_image_size": "side of the square network input", "train_epochs": "passes over the records (default: endless)",
    "max_number_of_steps": "global step at which training ends", "batch_size": "images per step",
    "tf_random_seed": "seed of the initialisers, the record shuffle and the augmentation draws",
    "checkpoint_path": "checkpoint (prefix or directory) to warm-start from when model_dir holds none",
    "checkpoint_model_scope": "model scope inside that checkpoint", "model_scope": "scope the variables are saved under",
    "checkpoint_exclude_scopes": "comma-separated scopes left at their initialisers on a warm start",
    "ignore_missing_vars": "a variable missing in the warm-start checkpoint keeps its initialiser",
    "num_classes": "2 (face / background): the only value the kernels implement",
}
_DAN_EXCLUDE = ("dan/predict_face, dan/prediction_modules_stage1, dan/prediction_modules_stage2, dan/predict_cascade, dan/additional_layers, "
                "dan/l2_norm_layer_3, dan/l2_norm_layer_4, dan/l2_norm_layer_5, dan/lfpn, dan/lfpn_stage1, dan/lfpn_stage2")
_DAN_FLAGS = dict(num_readers=24, num_preprocessing_threads=48, model_dir="./dan_logs/", batch_size=16, data_format="channels_last",
                  match_threshold=0.35, neg_threshold=0.35, decay_boundaries="50, 80000, 100000", model_scope="dan",
                  checkpoint_exclude_scopes=_DAN_EXCLUDE)
MODEL_FLAGS = {       # what each script's flag block changes against train_sfd.py's
    "sfd": {},
    "pb": dict(num_preprocessing_threads=48, model_dir="./pyramid_box_logs/", batch_size=14, model_scope="pyramid_box",
               checkpoint_exclude_scopes="pyramid_box/additional_layers, pyramid_box/l2_norm_layer_3, pyramid_box/l2_norm_layer_4, "
                                         "pyramid_box/l2_norm_layer_5, pyramid_box/lfpn, pyramid_box/cpm, pyramid_box/predict_face, "
                                         "pyramid_box/predict_head, pyramid_box/predict_body"),
    "dan": _DAN_FLAGS,
    "dan_deform": dict(_DAN_FLAGS, model_dir="./dan_logs_deform/"),       # train_dan_deform.py differs in the backbone import and this flag
}
# tensors_to_log of each script, in its order
LOG_KEYS = {"sfd": ("lr", "ce", "loc", "loss", "l2", "acc"),
            "pb": ("lr", "ce", "lc", "hce", "hlc", "bce", "blc", "ls", "wd", "acc"),
            "dan": ("lr", "ce", "loc", "ce2", "loc2", "loss", "l2", "acc")}
LOG_KEYS["dan_deform"] = LOG_KEYS["dan"]
NAME_REMAP = {"/conv2d/kernel": "/weights", "/conv2d/bias": "/biases"}     # get_init_fn of every script (train_sfd.py:159-163)
ANCHOR_SCALES = [16, 32, 64, 128, 256, 512]                                 # data-anchor-sampling scales (train_pb.py:203, train_dan.py:205)
KEEP_CHECKPOINT_MAX = 5                                                     # RunConfig(keep_checkpoint_max=5), train_sfd.py:476
PREFETCH_DEPTH = 2
MAX_THREADS = 16
LFPN_UPSAMPLE = ("bilinear", "transposed")                                  # --lfpn_upsample (net/pb_net.py LFPN_UPSAMPLE)
BACKBONES = ("vgg16", "resnet50", "resnet101", "resnet152")                 # --backbone (train_dan.BACKBONES)


def flag_defaults(model):
    d = collections.OrderedDict(REFERENCE_FLAGS)
    d.update(MODEL_FLAGS[model])
    return d


def _flag_bool(v):
    if v.lower() in ("true", "t", "1", "yes"):
        return True
    if v.lower() in ("false", "f", "0", "no"):
        return False
    raise argparse.ArgumentTypeError("expected true or false, got %r" % v)


def build_parser(model):
    p = argparse.ArgumentParser(prog="python -m dan_amd.train_%s" % model,
                                description="Train %s from TFRecords to TF-V2 checkpoints on one MI355X." % model)
    for name, default in flag_defaults(model).items():
        ignored = name in IGNORED_FLAGS
        text = "accepted for the reference's command lines and ignored" if ignored else _HELP.get(name, "as the reference's flag")
        if isinstance(default, bool):
            p.add_argument("--" + name, type=_flag_bool, nargs="?", const=True, default=default, metavar="BOOL", help=text + " (default %s)" % default)
        elif name in _INT_FLAGS:
            p.add_argument("--" + name, type=int, default=default, help=text + " (default %s)" % default)
        else:
            p.add_argument("--" + name, type=type(default), default=default, help=text + " (default %r)" % default)
    p.add_argument("--device", default="cuda:0", help="the GPU to train on (default cuda:0)")
    p.add_argument("--deterministic", action="store_true", help="bit-reproducible steps (every model of these drivers has an ordered form; dan_deform takes it through ops.deterministic_context())")
    p.add_argument("--decode_entropy", choices=("host", "device"), default="host", help="where the JPEG Huffman stage runs (default host)")
    p.add_argument("--no_checkpoint_checksums", action="store_true",
                   help="write checkpoints without per-tensor CRCs and do not verify the ones that are read (default: both, on the device)")
    p.add_argument("--no_prefetch", action="store_true", help="prepare each batch between the steps instead of on the background thread")
    if model != "sfd":                                                      # (S3FD has no LFPN)
        p.add_argument("--lfpn_upsample", choices=LFPN_UPSAMPLE, default="bilinear",
                       help="how the LFPN brings the upper level to the lateral's size: bilinear resize (the reference's graph, default) or a "
                            "learnable 4x4 stride-2 transposed convolution (new variables <lfpn>/fpn_k/upsample_deconv/{kernel,bias})")
    if model == "dan":                                                      # (the reference has no deformable ResNet backbone)
        p.add_argument("--backbone", choices=BACKBONES, default="vgg16",
                       help="vgg16 (the reference's script, default) or the reference's ResNet-50/101/152 backbone with batch norm; a ResNet starts "
                            "from seeded initialisers or resumes from model_dir (no warm start: --checkpoint_path maps VGG names only) and has no "
                            "--deterministic form")
    return p


def parse_comma_list(text):
    return [float(s.strip()) for s in text.split(",")]


def format_log(values):
    """The formatter of the reference's LoggingTensorHook (train_sfd.py:508-509)."""
    return ", ".join(["%s=%.6f" % (k, v) for k, v in values.items()])


# ------------------------------------------------------------------------------------------------------------ checkpoints
class CheckpointKeeper(object):
    """tf.train.Saver(max_to_keep=keep)'s bookkeeping in model_dir: the text state file `checkpoint` (model_checkpoint_path +
    all_model_checkpoint_paths, oldest first - the CheckpointState text proto that tf.train.latest_checkpoint and
    utility.checkpoint.latest_checkpoint both parse) and the removal of the files of checkpoints that fall off the list."""

    def __init__(self, model_dir, keep=KEEP_CHECKPOINT_MAX):
        self.model_dir, self.keep = model_dir, int(keep)
        self.kept = []
        state = os.path.join(model_dir, "checkpoint")
        if os.path.exists(state):
            for line in open(state):
                k, _, v = line.strip().partition(":")
                name = v.strip().strip('"')
                if k == "all_model_checkpoint_paths" and name and name not in self.kept:
                    self.kept.append(name)

    def prefix(self, step):
        return os.path.join(self.model_dir, "model.ckpt-%d" % step)

    def register(self, prefix):
        """`prefix`'s files have been written: it becomes the newest; the oldest beyond `keep` lose their files."""
        name = os.path.basename(prefix)
        self.kept = [n for n in self.kept if n != name] + [name]
        while len(self.kept) > self.keep:
            old = os.path.join(self.model_dir, self.kept.pop(0))
            for f in os.listdir(self.model_dir):
                if f == os.path.basename(old) + ".index" or f.startswith(os.path.basename(old) + ".data-"):
                    os.remove(os.path.join(self.model_dir, f))
        tmp = os.path.join(self.model_dir, "checkpoint.tmp")
        with open(tmp, "w") as f:
            f.write('model_checkpoint_path: "%s"\n' % name)
            for n in self.kept:
                f.write('all_model_checkpoint_paths: "%s"\n' % n)
        os.replace(tmp, os.path.join(self.model_dir, "checkpoint"))


# ------------------------------------------------------------------------------------------------------------ the models
class _Setup(object):
    """What the loop needs from one model: the trainer, the batched augmentation, the batch's anchor encoder and the log line's values."""

    def __init__(self, model, args, device, trainer_kw):
        import torch
        from .train_sfd import AnchorConfig
        size = args.train_image_size
        shape = (size, size)
        seed = args.tf_random_seed
        if model == "sfd":
            from .preprocessing import sfd_preprocessing as P
            from .train_sfd import SFDModel, SFDTrainer
            anchors = AnchorConfig(size, size, device, args.match_threshold, args.neg_threshold)
            self.trainer = SFDTrainer(SFDModel(device=device, seed=seed), **trainer_kw)
            self.preprocess = lambda images, boxes, draws: P.preprocess_batch_for_train(images, boxes, shape, draws=draws)
            self.encode = lambda boxes: anchors.encode_batch(boxes)[:2]                   # loc_targets, cls_targets
        elif model == "pb":
            from .preprocessing import pb_preprocessing as P
            from .train_pb import PBAnchorTargets, PBModel, PBTrainer
            targets = PBAnchorTargets(size, size, device)
            if (args.match_threshold, args.neg_threshold) != (0.4, 0.4):
                targets.face = AnchorConfig(size, size, device, args.match_threshold, args.neg_threshold)
            self.trainer = PBTrainer(PBModel(device=device, seed=seed, lfpn_upsample=args.lfpn_upsample), **trainer_kw)
            self.preprocess = lambda images, boxes, draws: P.preprocess_batch_for_train(images, boxes, shape, ANCHOR_SCALES, draws=draws)
            self.encode = lambda boxes: (targets.encode_batch(boxes),)
        else:
            from .preprocessing import dan_preprocessing as P
            from .train_dan import DANModel, DANTrainer, encode_batch_dan
            anchors = AnchorConfig(size, size, device, args.match_threshold, args.neg_threshold, ratios=_dan_ratios())
            self.trainer = DANTrainer(DANModel(device=device, seed=seed, deform=(model == "dan_deform"), lfpn_upsample=args.lfpn_upsample,
                                               backbone=getattr(args, "backbone", "vgg16")), anchors, routing_seed=seed,
                                      **deterministic_route(model, trainer_kw))
            self.preprocess = lambda images, boxes, draws: P.preprocess_batch_for_train(images, boxes, shape, ANCHOR_SCALES, draws=draws)
            self.encode = lambda boxes: encode_batch_dan(anchors, boxes)
        self.model = model
        self._torch = torch

    def log_values(self):
        """tensors_to_log of the model's script (one synchronising read of the loss terms, one of the metric)."""
        t = self.trainer
        v = t.loss_values()
        lr, acc = t._step_lr, t.metric_values()["cls_accuracy"]
        if self.model == "sfd":
            vals = (lr, v["face"][0], v["face"][1], v["total"], v["l2"], acc)
        elif self.model == "pb":
            vals = (lr, v["face"][0], v["face"][1], v["head"][0], v["head"][1], v["body"][0], v["body"][1], v["total"], v["l2"], acc)
        else:
            vals = (lr, v["stage1"][0], v["stage1"][1], v["stage2"][0], v["stage2"][1], v["total"], v["l2"], acc)
        return collections.OrderedDict(zip(LOG_KEYS[self.model], vals))


def deterministic_route(model, trainer_kw):
    """The trainer keywords --deterministic turns into.  The trainer's own flag covers the models whose every op had an ordered form when it
    was introduced; DAN-Deform (the deformable backward's ordered far-corner path) takes the context route instead: the same mode, asked for
    with ops_ctx=ops.deterministic_context()."""
    kw = dict(trainer_kw)
    if model == "dan_deform" and kw.get("deterministic"):
        from . import ops
        kw["deterministic"] = False
        kw["ops_ctx"] = ops.deterministic_context(kw.get("ops_ctx"))
    return kw


def _dan_ratios():
    from .train_dan import DAN_ANCHOR_RATIOS
    return DAN_ANCHOR_RATIOS


# ------------------------------------------------------------------------------------------------------------ input
def batches(setup, args, device, seed=None):
    """The plain generator of train_step argument tuples: slim_get_batch (records drawn from the shuffle buffer, JPEGs decoded on the device
    in groups of batch_size, each group augmented in one device pass) -> the images stacked to [B, S, S, 8] network input, the batch's boxes
    encoded against the anchors in one call.  Everything is launched on the CURRENT stream of the calling thread."""
    import numpy as np
    import torch
    from .dataset import dataset_common
    from .preprocessing.dan_preprocessing import Draws
    seed = args.tf_random_seed if seed is None else seed
    draws = Draws(seed)

    def prep_batch(images, bboxes_list):                                  # records hold normalised boxes, the augmentation takes pixels
        px = [np.asarray(b, np.float32).reshape(-1, 4) * np.asarray([im.shape[0], im.shape[1]] * 2, np.float32) for im, b in zip(images, bboxes_list)]
        return setup.preprocess(images, px, draws)

    gen = dataset_common.slim_get_batch(args.num_classes, args.batch_size, "train", os.path.join(args.data_dir, "{}-*"),
                                        min(args.num_readers, MAX_THREADS), min(args.num_preprocessing_threads, MAX_THREADS), None,
                                        lambda gbboxes: (gbboxes,), num_epochs=args.train_epochs, is_training=True, seed=seed,
                                        decode_device=device, decode_entropy=args.decode_entropy, batch_preprocessing_fn=prep_batch)
    for batch in gen:
        images = torch.stack([e[0] for e in batch])
        boxes = [torch.from_numpy(np.ascontiguousarray(e[3], dtype=np.float32)) for e in batch]
        yield (images,) + tuple(setup.encode(boxes))


def _tensors(tree):
    if hasattr(tree, "record_stream"):
        yield tree
    elif isinstance(tree, dict):
        for v in tree.values():
            yield from _tensors(v)
    elif isinstance(tree, (list, tuple)):
        for v in tree:
            yield from _tensors(v)


class Prefetcher(object):
    """One background thread runs `make_iter()` - record read, host Huffman stage, uploads, decode / augmentation / encoding launches - on a
    stream of its own, at most `depth` batches ahead; a batch is handed over with an event the consumer's stream waits for (no host wait),
    and its tensors are marked as used on that stream so the allocator does not hand their memory back to the loader early.  Same batches,
    same order, same bits as iterating make_iter() directly."""
    _END = object()

    def __init__(self, make_iter, device, depth=PREFETCH_DEPTH):
        import torch
        self._torch, self._make_iter, self._device = torch, make_iter, torch.device(device)
        self._q = queue.Queue(maxsize=depth)
        self._stop = threading.Event()
        self._stream = torch.cuda.Stream(self._device)
        self._thread = threading.Thread(target=self._run, name="danhip-prefetch", daemon=True)
        self._thread.start()

    def _put(self, item):
        while not self._stop.is_set():
            try:
                self._q.put(item, timeout=0.05)
                return True
            except queue.Full:
                pass
        return False

    def _run(self):
        torch = self._torch
        try:
            torch.cuda.set_device(self._device)
            with torch.cuda.stream(self._stream):
                for batch in self._make_iter():
                    ready = torch.cuda.Event()
                    ready.record(self._stream)
                    if not self._put((batch, ready)):
                        return
            self._put(self._END)
        except BaseException as e:                                          # raised again in the consumer
            self._put(e)

    def __iter__(self):
        torch = self._torch
        while True:
            item = self._q.get()
            if item is self._END:
                return
            if isinstance(item, BaseException):
                raise item
            batch, ready = item
            main = torch.cuda.current_stream(self._device)
            main.wait_event(ready)
            for t in _tensors(batch):
                t.record_stream(main)
            yield batch

    def close(self):
        self._stop.set()
        while self._thread.is_alive():
            try:
                self._q.get_nowait()                                        # a producer blocked on a full queue sees the stop flag
            except queue.Empty:
                pass
            self._thread.join(timeout=0.05)
        self._stream.synchronize()


# ------------------------------------------------------------------------------------------------------------ main
def _warm_start_path(path):
    from .utility import checkpoint
    if not path:
        return None
    if os.path.isdir(path):
        return checkpoint.latest_checkpoint(path)
    return path if os.path.exists(path + ".index") else None


def main(argv=None, model="sfd"):
    args = build_parser(model).parse_args(argv)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("dan_amd.train_%s trains on one GPU: WORLD_SIZE=%s is not supported here (bench.py --gpus N runs the multi-rank step)"
                         % (model, os.environ["WORLD_SIZE"]))
    if args.num_classes != 2:
        raise SystemExit("--num_classes %d: the loss and metric kernels are two-way (face / background)" % args.num_classes)
    from .utility import checkpoint
    backbone = getattr(args, "backbone", "vgg16")
    if backbone != "vgg16":                                                   # refused here, before the device is touched
        if args.deterministic:
            raise SystemExit("--deterministic with --backbone %s: batch norm has no ordered (bit-reproducible) form" % backbone)
        if not checkpoint.latest_checkpoint(args.model_dir) and _warm_start_path(args.checkpoint_path):
            raise SystemExit("--backbone %s cannot warm-start from --checkpoint_path %s: the checkpoint name mapping covers the VGG-16 variables only "
                             "(train from the seeded initialisers, or resume from --model_dir)" % (backbone, args.checkpoint_path))
    import torch
    device = torch.device(args.device)
    torch.cuda.set_device(device)
    os.makedirs(args.model_dir, exist_ok=True)
    trainer_kw = dict(weight_decay=args.weight_decay, negative_ratio=args.negative_ratio, momentum=args.momentum, base_lr=args.learning_rate,
                      lr_boundaries=tuple(int(b) for b in parse_comma_list(args.decay_boundaries)),
                      lr_factors=tuple(parse_comma_list(args.lr_decay_factors)), end_lr=args.end_learning_rate,
                      deterministic=args.deterministic, metrics=True)
    setup = _Setup(model, args, device, trainer_kw)
    trainer = setup.trainer
    keeper = CheckpointKeeper(args.model_dir)
    log_path = os.path.join(args.model_dir, "train.log")

    def say(text):
        print(text, flush=True)
        with open(log_path, "a") as f:
            f.write(text + "\n")

    scope_in_ckpt = None if args.checkpoint_model_scope in (None, "None") else args.checkpoint_model_scope
    found = checkpoint.latest_checkpoint(args.model_dir)
    warm = None if found else _warm_start_path(args.checkpoint_path)
    checked = not args.no_checkpoint_checksums                                # CRCs written ("device": the shard is checksummed on the GPU) and verified
    if found:
        trainer.restore(found, args.model_scope, verify=checked)
        print("resumed %s at step %d" % (found, trainer.step_no), flush=True)
    elif warm:
        names = checkpoint.init_from_checkpoint(trainer.model.vs, warm, args.model_scope, scope_in_ckpt, args.checkpoint_exclude_scopes,
                                                args.ignore_missing_vars, name_remap=NAME_REMAP, verify=checked)
        print("warm start from %s: %d variables" % (warm, len(names)), flush=True)
    else:
        print("no checkpoint in %s or at %s: seeded initialisers (%d)" % (args.model_dir, args.checkpoint_path, args.tf_random_seed), flush=True)

    make_iter = lambda: batches(setup, args, device)
    loader = None if args.no_prefetch else Prefetcher(make_iter, device)
    saved_at = trainer.step_no if found else None
    done = 0
    try:
        for batch in (loader if loader is not None else make_iter()):
            if trainer.step_no >= args.max_number_of_steps:
                break
            trainer.train_step(*batch)
            step = trainer.step_no
            if done % max(args.log_every_n_steps, 1) == 0:                  # LoggingTensorHook(every_n_iter): the run's first step, then every n-th
                say("step %d: %s" % (step, format_log(setup.log_values())))
            done += 1
            if args.save_checkpoints_steps > 0 and step % args.save_checkpoints_steps == 0:
                trainer.save(keeper.prefix(step), args.model_scope, checksums="device" if checked else False)
                keeper.register(keeper.prefix(step))
                saved_at = step
            if step >= args.max_number_of_steps:
                break
        if saved_at != trainer.step_no:                                      # the Estimator's CheckpointSaverHook.end
            trainer.save(keeper.prefix(trainer.step_no), args.model_scope, checksums="device" if checked else False)
            keeper.register(keeper.prefix(trainer.step_no))
    finally:
        if loader is not None:
            loader.close()
        trainer.close()
    return 0
