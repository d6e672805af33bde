"""CPU checks of the fused image training step (include/dpt_hip.h "image training step",
csrc/dpt_imagestep.hip, dpt_hip.train.DeviceImageData / ImageTrainer, train_miniworld.py --fused): the new
symbols and dpt_image_data's layout, the step workspace against a Python restatement, every host check
failing before a launch with a message, the CLI's guards with --fused, and the new source under the ISA
hazard scan and without scratch.  No device work is launched."""
import ctypes
import os
import shutil
import subprocess

import pytest

from conftest import ROOT
from test_image_host import _numel_py as front_ws_numel
from test_isa_hazards import HIPCC, test_no_short_mfma_hazard_paths as hazard_scan
from test_resource_budget import remarks

NEW_SYMBOLS = ("dpt_image_normalize", "dpt_image_pack_batch", "dpt_image_train_step_workspace_numel",
               "dpt_image_train_step", "dpt_image_train_eval_loss")


def _lib():
    from dpt_hip import _lib
    return _lib, _lib.load()


def test_new_symbols_and_abi_version():
    L, lib = _lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in L.SIGNATURES, name
    assert lib.dpt_abi_version() == 8 == L.ABI_VERSION
    from dpt_hip import train as tr
    assert hasattr(tr, "DeviceImageData") and hasattr(tr, "ImageTrainer")


def test_image_data_layout_matches_header(tmp_path):
    L, _ = _lib()
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dpt_hip.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(dpt_image_data));']
    for fname, _t in L.ImageData._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(dpt_image_data, {fname}));')
    lines.append("return 0; }")
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")],
                   check=True)
    got = dict(line.rsplit(" ", 1) for line in subprocess.run([str(tmp_path / "layout")], check=True,
                                                              capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(L.ImageData) == 72
    assert [f for f, _t in L.ImageData._fields_] == ["n", "horizon", "image_size", "query_states", "context_states",
                                                     "context_actions", "context_rewards", "optimal_actions",
                                                     "query_images", "context_images"]
    for fname, _t in L.ImageData._fields_:
        assert int(got[fname]) == getattr(L.ImageData, fname).offset, fname


# ----------------------------------------------------------------------------- workspace
def _train_desc(L, n_layer=2, E=32, sd=2, A=4, B=5, T=4, flags=0, dropout=0.0, seed=0):
    return L.TrainDesc(n_layer, E, sd, A, 4 * T, B, T, flags, dropout, 0, seed)


@pytest.mark.parametrize("n_layer,E,sd,A,B,T", [(2, 32, 2, 4, 5, 4), (2, 18, 2, 4, 3, 4), (1, 7, 1, 3, 1, 1),
                                                (4, 32, 2, 4, 64, 51)])
def test_step_workspace_numel(n_layer, E, sd, A, B, T):
    """the regions of csrc/dpt_imagestep.hip ImageStepWs restated: images, feats, targets, embeds, dembeds,
    preds, dpreds, the front workspace (test_image_host's restatement of it), the trunk workspace and the
    two gradient blobs (the library's own, pinned elsewhere), B doubles; each rounded up to 4 floats"""
    L, lib = _lib()
    r4 = lambda n: (n + 3) & ~3  # noqa: E731
    d = _train_desc(L, n_layer, E, sd, A, B, T)
    n, tw, nb = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    assert lib.dpt_image_train_step_workspace_numel(ctypes.byref(d), ctypes.byref(n)) == 0
    assert lib.dpt_train_workspace_numel(ctypes.byref(d), ctypes.byref(tw)) == 0
    assert lib.dpt_train_blob_numel(ctypes.byref(d), ctypes.byref(nb)) == 0
    R, G = B * T, sd + A + 1
    nfront = 432 + 16 + 2304 + 16 + 1600 * 8 + 8 + (8 + G) * E + 3 * E
    want = (r4(R * 1875) + r4(R * G) + r4(B * A) + 2 * r4(R * E) + 2 * r4(R * A)
            + r4(front_ws_numel(R, sd, A, E, False)) + r4(tw.value) + r4(nfront) + r4(nb.value) + r4(2 * B))
    assert n.value == want
    # the forward-only chain uses the same regions: its two workspaces are no larger
    fo = _train_desc(L, n_layer, E, sd, A, B, T, flags=L.TRAIN_FORWARD_ONLY)
    two = ctypes.c_int64()
    assert lib.dpt_train_workspace_numel(ctypes.byref(fo), ctypes.byref(two)) == 0
    assert two.value <= tw.value and front_ws_numel(R, sd, A, E, True) <= front_ws_numel(R, sd, A, E, False)


# ----------------------------------------------------------------------------- host checks
def test_host_checks_without_a_device():
    """Every check fails on the host before any launch: the pointers below are host memory that a kernel
    would fault on, and no device is needed to get the exception types."""
    L, lib = _lib()
    buf = (ctypes.c_double * 64)()
    base = (ctypes.addressof(buf) + 15) & ~15
    p, q, odd = ctypes.c_void_p(base), ctypes.c_void_p(base + 64), ctypes.c_void_p(base + 4)
    H = 3
    d = _train_desc(L)
    data = L.ImageData(5, H, 25, *([p.value] * 7))
    opt = L.AdamWArgs(1e-3, 0.9, 0.999, 1e-8, 1e-4, 1)
    n = ctypes.c_int64()

    def step(desc=d, dat=data, index=p, perm=None, batch=5, trunk=p, tm=p, tv=p, front=q, fm=p, fv=p, args=opt,
             ws=p, acc=p):
        L.call("dpt_image_train_step", ctypes.byref(desc) if desc is not None else None,
               ctypes.byref(dat) if dat is not None else None, index, perm, batch, trunk, tm, tv, front, fm, fv,
               ctypes.byref(args) if args is not None else None, ws, acc, None)

    def evl(desc=d, dat=data, index=p, perm=None, batch=5, trunk=p, front=q, ws=p, acc=p):
        L.call("dpt_image_train_eval_loss", ctypes.byref(desc) if desc is not None else None,
               ctypes.byref(dat) if dat is not None else None, index, perm, batch, trunk, front, ws, acc, None)

    # null pointers, each in turn
    for kw in (dict(desc=None), dict(dat=None), dict(index=None), dict(trunk=None), dict(tm=None), dict(tv=None),
               dict(front=None), dict(fm=None), dict(fv=None), dict(args=None), dict(ws=None), dict(acc=None)):
        with pytest.raises(ValueError, match="null"):
            step(**kw)
    for kw in (dict(desc=None), dict(dat=None), dict(index=None), dict(trunk=None), dict(front=None), dict(ws=None),
               dict(acc=None)):
        with pytest.raises(ValueError, match="null"):
            evl(**kw)
    no_images = L.ImageData(5, H, 25, *([p.value] * 6), None)
    for call in (step, evl):
        with pytest.raises(ValueError, match="null dataset array"):
            call(dat=no_images)
        # the batch
        for batch in (0, -1, 6):
            with pytest.raises(ValueError, match="batch"):
                call(batch=batch)
        # window != 1 + horizon
        with pytest.raises(ValueError, match="window"):
            call(dat=L.ImageData(5, H + 1, 25, *([p.value] * 7)))
        with pytest.raises(ValueError, match="window"):
            call(desc=_train_desc(L, T=5))
        # image sizes other than 25 are not built
        with pytest.raises(NotImplementedError, match="image_size"):
            call(dat=L.ImageData(5, H, 24, *([p.value] * 7)))
        with pytest.raises(NotImplementedError, match="action_dim"):
            call(desc=_train_desc(L, A=33))
        with pytest.raises(ValueError, match="flags"):
            call(desc=_train_desc(L, flags=L.TRAIN_FORWARD_ONLY))
        with pytest.raises(ValueError, match="16-byte aligned"):
            call(ws=odd)
        with pytest.raises(ValueError, match="16-byte aligned"):
            call(front=odd)
        with pytest.raises(ValueError, match="one buffer"):
            call(front=p)
        with pytest.raises(ValueError, match="dropout"):
            call(desc=_train_desc(L, dropout=1.0))
    with pytest.raises(ValueError, match="step"):
        step(args=L.AdamWArgs(1e-3, 0.9, 0.999, 1e-8, 1e-4, 0))

    # the normalise call
    for args in ((None, 0, 1, p), (p, 0, 1, None)):
        with pytest.raises(ValueError, match="null"):
            L.call("dpt_image_normalize", *args, None)
    for code in (-1, 2, 7):
        with pytest.raises(ValueError, match="dtype"):
            L.call("dpt_image_normalize", p, code, 1, p, None)
    with pytest.raises(ValueError, match="n_images"):
        L.call("dpt_image_normalize", p, 0, -1, p, None)
    assert lib.dpt_image_normalize(p, 1, 0, p, None) == 0  # nothing to do, nothing launched

    # the pack call
    for hole in range(6):
        args = [ctypes.byref(d), ctypes.byref(data), p, None, 5, p, p, p]
        args[hole if hole < 3 else hole + 2] = None
        with pytest.raises(ValueError, match="null"):
            L.call("dpt_image_pack_batch", *args, None)
    with pytest.raises(ValueError, match="window"):
        L.call("dpt_image_pack_batch", ctypes.byref(_train_desc(L, T=5)), ctypes.byref(data), p, None, 5, p, p, p, None)
    with pytest.raises(NotImplementedError, match="image_size"):
        L.call("dpt_image_pack_batch", ctypes.byref(d), ctypes.byref(L.ImageData(5, H, 32, *([p.value] * 7))), p, None, 5,
               p, p, p, None)
    with pytest.raises(ValueError, match="batch"):
        L.call("dpt_image_pack_batch", ctypes.byref(d), ctypes.byref(data), p, None, 0, p, p, p, None)

    # the workspace size
    with pytest.raises(ValueError, match="null"):
        L.call("dpt_image_train_step_workspace_numel", ctypes.byref(d), None)
    with pytest.raises(ValueError, match="null"):
        L.call("dpt_image_train_step_workspace_numel", None, ctypes.byref(n))
    with pytest.raises(ValueError, match="batch"):
        L.call("dpt_image_train_step_workspace_numel", ctypes.byref(_train_desc(L, B=0)), ctypes.byref(n))


def test_train_miniworld_fused_keeps_the_cli_guards(tmp_path, monkeypatch):
    import importlib
    tm = importlib.import_module("train_miniworld")
    monkeypatch.chdir(tmp_path)
    with pytest.raises(NotImplementedError, match="miniworld"):
        tm.main(["--env", "bandit", "--fused"])
    assert not os.path.exists(tmp_path / "datasets")
    # --workers' help says that the fused path ignores it
    import contextlib
    import io
    out = io.StringIO()
    with pytest.raises(SystemExit), contextlib.redirect_stdout(out):
        tm.main(["--help"])
    text = " ".join(out.getvalue().split())
    assert "--fused" in text and "ignored with --fused" in text


# ----------------------------------------------------------------------------- the new source
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_imagestep_source_passes_the_hazard_scan(tmp_path):
    hazard_scan("dpt_imagestep.hip", tmp_path)
    assert "dpt_imagestep.hip" in open(os.path.join(ROOT, "decision-pretrained-transformer_amd", "csrc",
                                                    "Makefile")).read()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_imagestep_kernels_use_no_scratch(tmp_path):
    r = remarks("dpt_imagestep.hip", tmp_path)
    names = [n for n in r if "is_normalize" in n or "is_pack" in n]
    assert len(names) == 3, list(r)  # the float64 and float32 normalise kernels and the gather
    for n in names:
        assert r[n]["scratch"] == 0 and r[n]["occ"] >= 2, (n, r[n])
