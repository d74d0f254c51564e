"""The one recipe behind every native test: tests/native/<driver> and the csrc files it needs are compiled for the CPU by g++,
with AddressSanitizer and UndefinedBehaviorSanitizer, into a stand-alone program with its own main, and that program is run in
a child process whose output is held to one predicate.  Nothing sanitised is loaded into Python.  This is the only place under
tests/ that names a compiler flag, a sanitizer option or a report string; the modules import it as they import jpeg_cases."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO

CSRC = os.path.join(REPO, "poserisk_release_amd", "csrc")
NATIVE = os.path.join(REPO, "tests", "native")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
SANITIZER_ENV = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"}
REPORTS = ("AddressSanitizer", "runtime error", "CHECK FAILED")


def clean(returncode, stderr):
    """The one predicate: the program ended with 0 and neither sanitizer nor a driver's CHECK reported anything."""
    return returncode == 0 and not any(word in stderr for word in REPORTS)


class Program:
    def __init__(self, exe, work_dir):
        self.exe, self.dir = exe, work_dir          # dir: where the tests put the program's input and output files

    def run(self, *args, timeout=1200, env=None, check=True):
        """-> CompletedProcess.  The child sees no POSERISK_* switch of the developer's (the drivers set the plan's switches
        themselves), the sanitizers' options, then `env`."""
        child = {k: v for k, v in os.environ.items() if not k.startswith("POSERISK_")}
        child.update(SANITIZER_ENV)
        child.update(env or {})
        r = subprocess.run([self.exe, *[str(a) for a in args]], capture_output=True, text=True, timeout=timeout, env=child)
        if check:
            assert clean(r.returncode, r.stderr), (r.returncode, r.stdout[-2000:], r.stderr[-6000:])
        return r


def build(tmp_dir, name, main, *, sources=(), stage=(), shim=False, threads=False, strict=False, sanitize=True,
          without_compiler="fail", staged_text=None):
    """Compiles tests/native/<main> plus `sources` (csrc files) into <tmp_dir>/<name> -> Program.
    stage: csrc files copied into tmp_dir, for the drivers that #include a .hip or .cc and for `sources` that must find the shim;
    shim: tests/native/host_shim.h goes beside them as common.h, which is what the staged kernels include;
    staged_text: {csrc file name: text} -- a staged file whose text is given here is written from it instead of being copied
        (tests/test_track_mutants_native.py builds mutated kernels this way: the text exists in tmp_dir only);
    without_compiler: "fail", "skip" or "none" (-> None) where there is no g++."""
    gxx = shutil.which("g++")
    if gxx is None:
        if without_compiler == "skip":
            pytest.skip("no g++")
        assert without_compiler == "none", f"g++ is needed to build tests/native/{main} for the host"
        return None
    d = str(tmp_dir)
    staged_text = dict(staged_text or {})
    assert set(staged_text) <= set(stage), "staged_text names a file that is not staged"
    for f in stage:
        if f in staged_text:
            with open(os.path.join(d, f), "w") as out:
                out.write(staged_text[f])
        else:
            shutil.copy(os.path.join(CSRC, f), os.path.join(d, f))
    if shim:
        shutil.copy(os.path.join(NATIVE, "host_shim.h"), os.path.join(d, "common.h"))
    exe = os.path.join(d, name)
    cmd = [gxx, "-std=c++17", "-O1", "-g", *(SANITIZE if sanitize else ()), *(("-Wall", "-Werror") if strict else ("-Wno-unknown-pragmas",)),
           *(("-pthread",) if threads else ()), "-x", "c++", "-I", d, "-I", CSRC, "-o", exe, os.path.join(NATIVE, main),
           *[os.path.join(d if f in stage else CSRC, f) for f in sources]]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    return Program(exe, tmp_dir)


def pack_streams(path, blobs):
    """int64 F | int64 offsets[F + 1] | the blobs back to back: what read_pack (tests/native/native_common.h) reads."""
    off = np.cumsum([0] + [len(b) for b in blobs]).astype(np.int64)
    with open(path, "wb") as f:
        f.write(np.int64(len(blobs)).tobytes() + off.tobytes() + b"".join(blobs))
    return path


def taker(path):
    """-> take(dtype, n): the next n items of the file, and take.done(): asserts that the file ended there."""
    raw, pos = np.fromfile(path, np.uint8), [0]

    def take(dtype, n):
        a = raw[pos[0]:pos[0] + n * np.dtype(dtype).itemsize].view(dtype)
        pos[0] += a.nbytes
        return a

    def done():
        assert pos[0] == raw.size
    take.done = done
    return take
