"""The smoothing kernel's source and its argument validation on the CPU, under ASan + UBSan.

`poserisk_release_amd/csrc/smooth.hip` is compiled unchanged for the host against `tests/native/host_shim.h` (a workgroup = 256
threads and a barrier, workgroups one after the other) into a stand-alone program, `tests/native/smooth_host.cc`, and run on
exact-size heap buffers over every case of tests/smooth_cases.py: every address the kernel forms -- the halo at a track's and a
tile's edge, the ragged last tile, the workspace -- is checked by the sanitizer, and the outputs against the float64
restatement of the contract (tests/smooth_ref.py) by the contract's tolerances.  `--validate` gives pr_smooth_tracks every
argument error in turn.  Nothing here is loaded into Python.  What this cannot show is anything about the GPU build itself --
tests/test_smooth_gpu.py does that."""
import pytest

import host_build
import smooth_cases as sc


@pytest.fixture(scope="module")
def smooth_host(tmp_path_factory):
    d = tmp_path_factory.mktemp("smooth_host")
    exe = host_build.build(d, "smooth_host", "smooth_host.cc", stage=("smooth.hip",), shim=True, threads=True)

    def run(name):
        exe.run(sc.write_case(d / "case.bin", name), d / "out.bin", sc.TILE)
        return sc.read_outputs(d / "out.bin", name)
    run.exe = exe
    return run


def test_every_argument_error_is_refused_before_any_work(smooth_host):
    assert "0 failures" in smooth_host.exe.run("--validate").stdout


@pytest.mark.parametrize("name", sc.NAMES)
def test_kernel_source_on_the_host_matches_the_reference(smooth_host, name):
    sc.check(name, smooth_host(name))


@pytest.mark.parametrize("name", sc.SWEEP_NAMES)
def test_the_seeded_sweep_on_the_host_matches_the_reference(smooth_host, name):
    sc.check(name, smooth_host(name))
