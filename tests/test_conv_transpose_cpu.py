"""What the transposed-convolution feature promises without a GPU: the exact cases satisfy the condition their equality rests on, the
reference counts taps as the rule says, the initialiser is the stated formula, the command lines carry the flag, the C ABI table carries
the entry points, and the host planning code survives the sanitizers."""
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_transpose_exact as CT  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = CT.all_cases()
ENTRY_POINTS = ("danhip_conv_transpose4x4s2_pack_weight", "danhip_conv_transpose4x4s2_add_fwd", "danhip_conv_transpose4x4s2_dgrad",
                "danhip_conv_transpose4x4s2_wgrad_workspace_bytes", "danhip_conv_transpose4x4s2_wgrad_slabs", "danhip_conv_transpose4x4s2_wgrad",
                "danhip_conv_transpose4x4s2_add_fwd_f32")


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_exact_cases_hold_integers_the_formats_keep(case):
    CT.check_inputs(case)


def test_case_list_covers_what_the_kernels_can_get_wrong():
    maps = {(c["Hi"], c["Wi"]) for c in CASES}
    assert {(1, 1), (1, 3), (3, 1), (5, 7), (9, 17)} <= maps
    assert 8 * 17 > CT.TILE_PIXELS > 7 * 17                                     # 9 x 17 crosses the flat 128-pixel tile inside its last rows
    for hw in CT.MAPS:
        for ch in CT.CHANNELS:
            for n in (1, 3):
                got = {c["Ho"] - 2 * c["Hi"] for c in CASES if (c["Hi"], c["Wi"]) == hw and (c["Cin"], c["Cout"]) == ch and c["N"] == n and c["kind"] == "random"}
                assert got == {0, -1}, (hw, ch, n)
    assert any(c["Cin"] == 512 and c["Cout"] == 512 and (c["Hi"], c["Wi"]) == (3, 5) for c in CASES)


@pytest.mark.parametrize("hw", [(1, 1), (1, 3), (3, 1), (5, 7)])
@pytest.mark.parametrize("crop", [False, True])
def test_reference_counts_one_two_or_four_taps(hw, crop):
    """All-ones x and W, zero bias: Cin x {1, 2, 4} at corner, edge and interior.  The expected map is written out by hand here - first and
    last row / column of the full 2 Hi x 2 Wi map have one tap per axis, all others two - and holds both the reference and CT.tap_counts."""
    Hi, Wi = hw
    Cin, Cout = 64, 64
    Ho, Wo = 2 * Hi - int(crop), 2 * Wi - int(crop)
    want = torch.empty((Ho, Wo), dtype=CT.F64)
    for oy in range(Ho):
        for ox in range(Wo):
            ny = 1 if oy in (0, 2 * Hi - 1) else 2
            nx = 1 if ox in (0, 2 * Wi - 1) else 2
            want[oy, ox] = Cin * ny * nx
    out = CT.reference(torch.ones((2, Hi, Wi, Cin)), torch.ones((4, 4, Cout, Cin)), torch.zeros(Cout), None, Ho, Wo)["out"]
    assert torch.equal(out, want[None, :, :, None].expand(2, Ho, Wo, Cout))
    cy, cx = torch.tensor(CT.tap_counts(Hi, Ho)), torch.tensor(CT.tap_counts(Wi, Wo))
    assert torch.equal((Cin * cy[:, None] * cx[None, :]).to(CT.F64), want)
    if Hi >= 3 and Wi >= 3:
        assert set(want.unique().tolist()) == {Cin, 2 * Cin, 4 * Cin}


def test_initialiser_is_the_bilinear_kernel():
    """kernel[ky, kx, co, ci] = f[ky] f[kx] delta(co, ci): equal to the formula, and the taps that reach one interior output sum to 1 (even
    outputs take ky in {1, 3}, odd ones {0, 2}: 0.75 + 0.25 per axis), so the initial operator interpolates."""
    from dan_amd.net.variables import VariableStore
    vs = VariableStore(device="cpu")
    k = vs.get("lfpn/fpn_1/upsample_deconv/kernel", (4, 4, 128, 128), "bilinear_deconv").detach()
    assert torch.equal(k.to(CT.F64), CT.deconv_initializer(128, 128))
    assert torch.equal(vs.get("lfpn/fpn_1/upsample_deconv/bias", (128,), "zeros").detach(), torch.zeros(128))
    for kys in ((1, 3), (0, 2)):
        for kxs in ((1, 3), (0, 2)):
            s = sum(k[ky, kx, 5, 5].item() for ky in kys for kx in kxs)
            assert s == 1.0
            assert sum(k[ky, kx, 5, 6].item() for ky in kys for kx in kxs) == 0.0
    # through the reference: a constant map stays constant in the interior; the border rows carry 0.75 (edge) and 0.5625 (corner) of it
    out = CT.reference(torch.ones((1, 3, 3, 64)), CT.deconv_initializer(64, 64), None, None, 6, 6)["out"][0, :, :, 0]
    assert torch.equal(out[1:5, 1:5], torch.ones((4, 4), dtype=CT.F64))
    assert out[0, 2].item() == 0.75 and out[0, 0].item() == 0.5625


def test_command_lines_carry_the_flag_and_nothing_else_changes():
    from dan_amd import eval_cli, train_cli
    for cli in (train_cli, eval_cli):
        for model in ("pb", "dan", "dan_deform"):
            p = cli.build_parser(model)
            assert p.parse_args([]).lfpn_upsample == "bilinear"
            assert p.parse_args(["--lfpn_upsample", "transposed"]).lfpn_upsample == "transposed"
            with pytest.raises(SystemExit):
                p.parse_args(["--lfpn_upsample", "nearest"])
            # the help text without the new option's entry is the help text of a parser that never had it
            text = p.format_help()
            assert "--lfpn_upsample {bilinear,transposed}" in text
            act = [a for a in p._actions if a.dest == "lfpn_upsample"][0]
            p._remove_action(act)
            for grp in p._action_groups:
                if act in grp._group_actions:
                    grp._group_actions.remove(act)
            rest = p.format_help()
            assert "lfpn_upsample" not in rest
            own = [a.dest for a in p._actions]
            assert own.index("device") > own.index("model_scope")                     # the reference's flags first, the port's own behind them
        assert not hasattr(cli.build_parser("sfd").parse_args([]), "lfpn_upsample")    # S3FD has no LFPN
    with pytest.raises(SystemExit, match="split"):
        eval_cli.main(["--lfpn_upsample", "transposed", "--precision", "split"], model="pb")
    for mod in (train_cli, eval_cli):
        assert "--lfpn_upsample" in mod.__doc__


def test_models_take_the_option_and_refuse_other_words():
    from dan_amd.net import pb_net
    from dan_amd.train_dan import DANModel
    from dan_amd.train_pb import PBModel
    assert pb_net.LFPN_UPSAMPLE == ("bilinear", "transposed")
    for cls in (PBModel, DANModel):
        assert cls(device="cpu").lfpn_upsample == "bilinear"
        assert cls(device="cpu", lfpn_upsample="transposed").lfpn_upsample == "transposed"
        with pytest.raises(ValueError):
            cls(device="cpu", lfpn_upsample="nearest")


def test_entry_points_are_in_the_table_and_the_library():
    from dan_amd import _lib
    for name in ENTRY_POINTS:
        assert name in _lib.PROTOTYPES, name
    L = _lib.lib()
    assert L.danhip_version() >= 19
    # the workspace query is a host function of the shape alone: more pixels than one slab's minimum -> more than one partial sum
    one = (1, 1, 1, 2, 2, 64, 64)
    many = (3, 9, 17, 18, 34, 64, 64)
    assert L.danhip_conv_transpose4x4s2_wgrad_slabs(*one) == 1 and L.danhip_conv_transpose4x4s2_wgrad_slabs(*many) > 1
    for dims in (one, many):
        slabs = L.danhip_conv_transpose4x4s2_wgrad_slabs(*dims)
        assert L.danhip_conv_transpose4x4s2_wgrad_workspace_bytes(*dims) >= slabs * 16 * 64 * 64 * 4 + 64 * 4
    assert L.danhip_conv_transpose4x4s2_wgrad_workspace_bytes(1, 1, 1, 2, 2, 72, 64) == 0
    assert L.danhip_conv_transpose4x4s2_wgrad_workspace_bytes(1, 1, 1, 3, 2, 64, 64) == 0


def test_checkpoint_without_the_new_variables_is_ignore_missing():
    from dan_amd.utility import checkpoint
    assert checkpoint._optional("pyramid_box/lfpn/fpn_1/upsample_deconv/kernel")
    assert checkpoint._optional("pyramid_box/lfpn/fpn_1/upsample_deconv/bias/Momentum")
    assert not checkpoint._optional("pyramid_box/lfpn/fpn_1/upsample_conv/kernel")


def test_host_planning_under_the_sanitizers(tmp_path):
    """tools/conv_transpose_plan_asan.cpp: a stand-alone program over the shape checks and the weight gradient's slab / workspace plan
    (dan_amd/csrc/conv_transpose_plan.h), built with -fsanitize=address,undefined and run on the CPU."""
    exe = str(tmp_path / "conv_transpose_plan_asan")
    src = os.path.join(ROOT, "tools", "conv_transpose_plan_asan.cpp")
    import shutil
    import warnings
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler (g++, c++, clang++): the box that built libdanhip has one"
    base = [cxx, "-std=c++17", "-O1", "-g"]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    is_clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static = [] if is_clang else ["-static-libasan", "-static-libubsan"]
    r = subprocess.run(base + san + static + [src, "-o", exe], capture_output=True, text=True)
    if r.returncode != 0:                       # as tests/test_jpeg_encode_cpu.py: the program's own checks remain
        warnings.warn("%s cannot link the sanitizer runtimes statically; conv_transpose_plan_asan runs WITHOUT sanitizers: %s" % (cxx, r.stderr[-300:]))
        r = subprocess.run(base + [src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "ok" in r.stdout
