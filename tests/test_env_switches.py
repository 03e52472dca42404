"""CPU: the shipped library and package read no A/B switches from the environment.  The native sources call no getenv at
all, the package's Python files name no MIVP_* variable outside an explicit allow-list, and no script under tools/ still
drives one of the removed switches (the variants they selected were last in commit 8154e35)."""
import glob
import os
import re

from conftest import ROOT

PKG = os.path.join(ROOT, "medical-image-segmentation-with-visual-prompts_amd")
ALLOWED = {"MIVP_FP8_ATTN_FWD"}                  # swin_ops.py: the fp8 forward experiment behind bench.py --fp8-attn
REMOVED = ["MIVP_ATTN_BWD_ABL", "MIVP_ATTN_BWD_REG_STAGING", "MIVP_ATTN_FWD_REG_STAGING", "MIVP_ATTN_MASK_CLASSES",
           "MIVP_ATTN_NO_XCD_REMAP", "MIVP_NO_WIDE_TOKEN_KERNELS", "MIVP_C48_QKV_ROW_KERNELS",
           "MIVP_QKV_FWD_STREAMED_WEIGHTS", "MIVP_GRAPH_FORCE_SINGLE"]


def _read(path):
    with open(path, errors="replace") as f:
        return f.read()


def test_native_sources_call_no_getenv():
    srcs = [p for p in glob.glob(os.path.join(PKG, "csrc", "*")) if os.path.isfile(p)]
    assert len(srcs) > 20
    assert [os.path.basename(p) for p in srcs if "getenv" in _read(p)] == []


def test_package_names_only_allowed_variables():
    srcs = glob.glob(os.path.join(PKG, "*.py")) + [os.path.join(ROOT, "mivp_amd.py")]
    assert len(srcs) > 20
    named = {m for p in srcs for m in re.findall(r"""["'](MIVP_[A-Z0-9_]+)["']""", _read(p))}
    assert named <= ALLOWED, sorted(named - ALLOWED)
    assert not set(REMOVED) & ALLOWED


def test_tools_drive_no_removed_switch():
    files = [p for p in glob.glob(os.path.join(ROOT, "tools", "**", "*"), recursive=True) if os.path.isfile(p)]
    assert len(files) > 20
    hits = [(os.path.relpath(p, ROOT), name) for p in files for name in REMOVED if name in _read(p)]
    assert hits == []
