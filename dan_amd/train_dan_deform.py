"""DAN-Deform training entry point - the reference's train_dan_deform.py, which differs from train_dan.py in two lines: the backbone import
(`from net import danet_deform as danet`, :27) and the model_dir flag's default ('./dan_logs_deform/', :54).  Here likewise: the model of
train_dan with deform=True, and the driver's "dan_deform" flag set.  --deterministic gives bit-reproducible steps here too: the driver
builds DANTrainer(DANModel(deform=True), anchors, ops_ctx=ops.deterministic_context()), and the deformable backward then takes its ordered
far-corner path (include/danhip.h).  The trainer's own deterministic=True keyword still refuses the deformable model."""
from .train_dan import DANModel, DANTrainer, dan_anchor_config, encode_batch_dan  # noqa: F401


class DANDeformModel(DANModel):
    def __init__(self, device="cuda", seed=20180817, lfpn_upsample="bilinear"):
        super().__init__(device=device, seed=seed, deform=True, lfpn_upsample=lfpn_upsample)


def main(argv=None):
    """`python -m dan_amd.train_dan_deform --data_dir D --model_dir M`: the reference's `python train_dan_deform.py ...` (dan_amd/train_cli.py)."""
    from .train_cli import main as run
    return run(argv, model="dan_deform")


if __name__ == "__main__":
    raise SystemExit(main())
