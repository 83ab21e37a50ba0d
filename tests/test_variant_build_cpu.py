"""The one build recipe (csrc/build.sh): a variant library built by its variant mode links, loads and exports what the product
exports; the scripts under tools/ keep no link line of their own and cite variant libraries only where the mode puts them."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "titok_video_amd", "csrc")
TOOLS = os.path.join(ROOT, "tools")


def _tool_files():
    for d, _dirs, files in os.walk(TOOLS):
        for f in sorted(files):
            try:
                yield os.path.relpath(os.path.join(d, f), ROOT), open(os.path.join(d, f)).read()
            except UnicodeDecodeError:      # a built ubench program
                pass


def _exports(path):
    nm = shutil.which("nm") or shutil.which("llvm-nm")
    out = subprocess.run([nm, "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return sorted(n for n in (line.split()[-1] for line in out.splitlines() if line.strip()) if n.startswith("ttv_"))


@pytest.mark.skipif(shutil.which("hipcc") is None or not os.path.exists(os.path.join(CSRC, "build", "ttv_api.o")),
                    reason="needs hipcc and the product objects of a finished build")
def test_noop_variant_links_loads_and_exports_the_product_set():
    """Variant `noop`: ttv_plan.hip (the quickest unit) recompiled with a -D nobody reads, every other object the product's."""
    lib = os.path.join(CSRC, "variants", "libtitok_hip_noop.so")
    obj = os.path.join(CSRC, "build", "ttv_plan__noop.o")
    had_dir = os.path.isdir(os.path.dirname(lib))
    stamps = {f: os.stat(os.path.join(CSRC, "build", f)).st_mtime_ns for f in os.listdir(os.path.join(CSRC, "build")) if f.endswith(".o") and "__" not in f}     # the product objects
    try:
        run = subprocess.run(["bash", os.path.join(CSRC, "build.sh"), "--variant", "noop", "ttv_plan", "-DTTV_VARIANT_NOOP=1"],
                             capture_output=True, text=True)
        assert run.returncode == 0, run.stdout + run.stderr
        assert run.stdout.strip().splitlines()[-1].endswith(lib), run.stdout       # it prints the path
        assert os.path.exists(lib) and os.path.exists(obj)
        for f, t in stamps.items():     # no product object was compiled again
            assert os.stat(os.path.join(CSRC, "build", f)).st_mtime_ns == t, f
        handle = ctypes.CDLL(lib)
        assert handle.ttv_version() >= 100
        from titok_video_amd import _lib
        product = os.path.join(ROOT, "titok_video_amd", "libtitok_hip.so")
        assert _exports(lib) == _exports(product) == sorted(_lib.SYMBOLS)
    finally:
        for p in (lib, obj):
            if os.path.exists(p):
                os.remove(p)
        if not had_dir and os.path.isdir(os.path.dirname(lib)) and not os.listdir(os.path.dirname(lib)):
            os.rmdir(os.path.dirname(lib))


def test_variant_mode_refuses_a_unit_the_object_list_does_not_name():
    """Refused before anything is compiled, so this needs neither hipcc nor a finished build."""
    for args in (["--variant", "x", "ttv_nosuch", "-DX"], ["--variant", "x"], ["--variant", "x", "-DX"]):
        run = subprocess.run(["bash", os.path.join(CSRC, "build.sh")] + args, capture_output=True, text=True)
        assert run.returncode == 2, (args, run.stdout + run.stderr)
    assert not os.path.exists(os.path.join(CSRC, "variants", "libtitok_hip_x.so"))


def test_object_list_flags_and_link_line_exist_once():
    text = open(os.path.join(CSRC, "build.sh")).read()
    assert text.count('HIP_SRCS="') == 1 and text.count('FLAGS="--offload-arch') == 1 and text.count("-shared") == 1
    assert "-Wl,--no-undefined" in text
    a64 = open(os.path.join(CSRC, "build_attn64.sh")).read()
    assert "FLAGS=" not in a64 and "$$" not in a64     # flags from build.sh, temporaries not named after the process


def test_tools_keep_no_link_line_of_their_own():
    for path, text in _tool_files():
        assert "-shared" not in text, path
        assert not re.search(r"build/ttv_\w+\.o", text), path
        if path.endswith(".sh") and os.path.dirname(path) == "tools":
            assert "hipcc" not in text and "offload-arch" not in text, path


def test_tools_cite_variant_libraries_under_variants_only():
    seen = 0
    for path, text in _tool_files():
        for m in re.finditer(r"[\w$/.{}()-]*libtitok_hip_[\w$<>{}*,]+\.so", text):
            seen += 1
            assert "csrc/variants/libtitok_hip_" in m.group(0), (path, m.group(0))
    assert seen > 20
