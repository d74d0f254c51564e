"""The activity kernels' source and their argument validation on the CPU, under ASan + UBSan.

`poserisk_release_amd/csrc/activity.hip` is compiled unchanged for the host against `tests/native/host_shim.h` (a workgroup =
its threads and a barrier, workgroups one after the other) into a stand-alone program, `tests/native/activity_host.cc`, and run
on exact-size heap buffers over every case of tests/activity_cases.py: every address the kernels form -- a chunk at a track's
start, the ragged last tile, the rows before the first, the workspace -- is checked by the sanitizer, and the outputs must EQUAL
the float64 restatement of the contract (tests/activity_ref.py).  `--validate` gives pr_activity_tracks every argument error in
turn.  Nothing here is loaded into Python.  What this cannot show is anything about the GPU build itself --
tests/test_activity_gpu.py does that."""
import pytest

import activity_cases as ac
import host_build


@pytest.fixture(scope="module")
def activity_host(tmp_path_factory):
    d = tmp_path_factory.mktemp("activity_host")
    exe = host_build.build(d, "activity_host", "activity_host.cc", stage=("activity.hip",), shim=True, threads=True)

    def run(name):
        exe.run(ac.write_case(d / "case.bin", name), d / "out.bin", ac.TILE, ac.CHUNK)
        return ac.read_outputs(d / "out.bin", name)
    run.exe = exe
    return run


def test_every_argument_error_is_refused_before_any_work(activity_host):
    assert "0 failures" in activity_host.exe.run("--validate").stdout


@pytest.mark.parametrize("name", ac.NAMES)
def test_kernel_source_on_the_host_equals_the_reference(activity_host, name):
    ac.check(name, activity_host(name))


@pytest.mark.parametrize("name", ac.SWEEP_NAMES)
def test_the_seeded_sweep_on_the_host_equals_the_reference(activity_host, name):
    ac.check(name, activity_host(name))
