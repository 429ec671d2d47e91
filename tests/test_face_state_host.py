"""The host side of the per-face extras (masks, guidance, previews, multistep history) without a GPU.

1. FaceSet (hifidiff_amd/csrc/hd_faceset.hpp): a stand-alone program with its own main that includes nothing but that header, built with
   the host C++ compiler -- with -fsanitize=address,undefined where the compiler can build and run such a program, plain otherwise (the
   test prints which) -- and run: it exits non-zero at the first failed check.
2. Denoiser and FacialRefiner share one base class: each still exposes exactly the public names it had before the base existed, and
   the shared methods (and so their docstrings) are one object on both."""
import os
import shutil
import subprocess

import pytest
from torch import nn

from conftest import ROOT

HEADER = os.path.join(ROOT, "hifidiff_amd", "csrc", "hd_faceset.hpp")

PROGRAM = r"""
#include "hd_faceset.hpp"
#include <cstdio>
#define CHECK(x) do { if (!(x)) { std::printf("line %d: %s\n", __LINE__, #x); return 1; } } while (0)
int main() {
    hdi::FaceSet s;
    // a new set and a dropped one are sized for no batch
    CHECK(!s.valid_for(0) && !s.valid_for(1) && s.count() == 0 && !s.any(1) && !s.all(1));
    // count under set, clear and re-set of the same slot; setting a slot twice counts once
    s.reset(3);
    CHECK(s.valid_for(3) && !s.valid_for(2) && !s.valid_for(4) && s.count() == 0 && !s.any(3) && !s.all(3));
    s.set(1, true);
    CHECK(s.count() == 1 && s.get(1) && !s.get(0) && !s.get(2));
    s.set(1, true);
    CHECK(s.count() == 1 && s.get(1));
    s.set(1, false);
    CHECK(s.count() == 0 && !s.get(1));
    s.set(1, false);
    CHECK(s.count() == 0);
    s.set(1, true);
    CHECK(s.count() == 1 && s.get(1));
    // any / all at B = 3 with one flag set: any for the batch it was sized for only, all not before every flag is set
    CHECK(s.any(3) && !s.all(3) && !s.any(2) && !s.any(4) && !s.all(1));
    s.set(0, true); s.set(2, true);
    CHECK(s.count() == 3 && s.all(3) && s.any(3) && !s.all(2) && !s.all(4));
    s.set(2, false);
    CHECK(s.count() == 2 && !s.all(3) && s.any(3));
    // reset to a different B: all clear, sized for the new batch only
    s.reset(5);
    CHECK(s.valid_for(5) && !s.valid_for(3) && s.count() == 0 && !s.any(5) && !s.any(3));
    for (int f = 0; f < 5; ++f) CHECK(!s.get(f));
    s.set(4, true);
    CHECK(s.count() == 1 && s.get(4) && s.any(5) && !s.all(5));
    s.reset(2);                                  // a smaller one
    CHECK(s.valid_for(2) && !s.valid_for(5) && s.count() == 0 && !s.get(0) && !s.get(1));
    // any / all at B = 1
    s.reset(1);
    CHECK(!s.any(1) && !s.all(1));
    s.set(0, true);
    CHECK(s.any(1) && s.all(1) && s.count() == 1 && !s.any(3) && !s.all(3));
    s.set(0, false);
    CHECK(!s.any(1) && !s.all(1) && s.count() == 0);
    // valid_for after drop: for no batch, whatever was set before
    s.set(0, true);
    s.drop();
    CHECK(!s.valid_for(1) && !s.valid_for(0) && s.count() == 0 && !s.any(1) && !s.all(1) && !s.all(0));
    s.reset(3);
    CHECK(s.valid_for(3) && s.count() == 0);
    return 0;
}
"""


def _compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    return None


def _sanitizer_flags(cxx, tmp):
    """-fsanitize=address,undefined if this compiler builds a trivial program with it that runs, else nothing."""
    src, exe = os.path.join(tmp, "probe.cpp"), os.path.join(tmp, "probe")
    with open(src, "w") as fh:
        fh.write("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    built = subprocess.run([cxx, "-std=c++17"] + flags + [src, "-o", exe], capture_output=True)
    if built.returncode == 0 and subprocess.run([exe], capture_output=True).returncode == 0:
        return flags
    return []


def test_faceset_standalone_program(tmp_path):
    cxx = _compiler()
    assert cxx, "no host C++ compiler (c++, g++ or clang++) on this machine"
    with open(HEADER) as fh:
        text = fh.read()
    assert not [ln for ln in text.splitlines() if ln.startswith("#include") and ("hip" in ln or '"' in ln)], "the header includes HIP or the project"
    tmp = str(tmp_path)
    flags = _sanitizer_flags(cxx, tmp)
    print("FaceSet program built with %s %s" % (cxx, " ".join(flags) if flags else "(no sanitizer: this compiler cannot build and run one)"))
    src, exe = os.path.join(tmp, "faceset_main.cpp"), os.path.join(tmp, "faceset_main")
    with open(src, "w") as fh:
        fh.write(PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + flags + ["-I", os.path.dirname(HEADER), src, "-o", exe],
                   check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stdout, run.stderr[-2000:])


# the public names of the two model classes beyond nn.Module's, as they were before the shared base class
DENOISER = ["check", "clear_guidance", "clear_mask", "cuda", "disable_guidance", "disable_previews", "enable_previews", "engine", "forward",
            "load_state_dict", "previews", "set_guidance", "set_mask", "state_dict", "to"]
REFINER = ["check", "clear_guidance", "clear_mask", "cuda", "disable_guidance", "disable_pool", "disable_previews", "enable_pool",
           "enable_previews", "engine", "forward", "invalidate_conditioning", "load_state_dict", "pool_commit", "pool_prepare", "prepare",
           "prepare_slots", "previews", "set_guidance", "set_mask", "state_dict", "to"]


def _public(cls):
    """Public names the class or one of the package's classes below it defines (nn.Module's own, unless overridden, are not counted)."""
    ours = [k for k in cls.__mro__ if k.__module__.startswith("hifidiff_amd")]
    return sorted(n for n in dir(cls) if not n.startswith("_") and any(n in k.__dict__ for k in ours))


def test_model_classes_keep_their_public_surface():
    from hifidiff_amd.refiner import Denoiser, FacialRefiner
    assert _public(Denoiser) == DENOISER
    assert _public(FacialRefiner) == REFINER
    assert issubclass(Denoiser, nn.Module) and issubclass(FacialRefiner, nn.Module)
    for name in ("set_mask", "set_guidance", "enable_previews"):
        a, b = getattr(Denoiser, name), getattr(FacialRefiner, name)
        assert a.__doc__ and a.__doc__ is b.__doc__, name
    # every public method documents itself once: the shared ones are the same function on both classes
    for name in sorted(set(DENOISER) & set(REFINER) - {"forward", "load_state_dict", "state_dict"}):
        assert getattr(Denoiser, name) is getattr(FacialRefiner, name), name


def test_argument_errors_still_come_first_without_a_batch():
    """set_mask / set_guidance on a model that has no prepared batch: a wrong argument is a ValueError, right ones a RuntimeError."""
    import torch
    from hifidiff_amd.refiner import Denoiser, FacialRefiner
    for cls in (Denoiser, FacialRefiner):
        m = cls(16)
        ok = torch.zeros((2, 4, 16, 16))
        with pytest.raises(ValueError):
            m.set_mask(torch.full((2, 16, 16), 2.0), ok, ok)
        with pytest.raises(RuntimeError, match="no batch is prepared"):
            m.set_mask(torch.ones((2, 16, 16)), ok, ok)
        with pytest.raises(ValueError):
            m.set_guidance(ok, 1.5, 4)
        with pytest.raises(RuntimeError, match="no batch is prepared"):
            m.set_guidance(ok, 0.5, 4)
        m.clear_mask()
        m.clear_guidance()
