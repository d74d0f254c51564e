"""host_build.clean, the one "was the run clean" predicate of the native tests, on canned output: nothing is compiled or run."""
import host_build

ASAN = """=================================================================
==4242==ERROR: AddressSanitizer: heap-buffer-overflow on address 0x602000000031 at pc 0x55d0c0de1234 bp 0x7ffc0 sp 0x7ffb8
READ of size 1 at 0x602000000031 thread T0
SUMMARY: AddressSanitizer: heap-buffer-overflow jpeg.hip:101 in get_bits
"""
UBSAN = "resize.hip:88:31: runtime error: signed integer overflow: 2147483647 + 1 cannot be represented in type 'int'\n"
CHECK = "CHECK FAILED tests/native/fence_check.cc:120: fp32_default B=37: tensor 3 of launch 12 does not end on its buffer\n"
WORDS = "null xofs_host\nevery side must lie in 1..4096\n"          # what a driver that provokes refusals prints


def test_a_clean_run_is_clean():
    assert host_build.clean(0, "") and host_build.clean(0, WORDS)


def test_each_kind_of_report_is_not():
    for stderr in (ASAN, UBSAN, CHECK):
        assert not host_build.clean(0, stderr) and not host_build.clean(0, WORDS + stderr + WORDS)
        assert not host_build.clean(1, stderr)


def test_a_failed_program_is_not_clean_even_when_silent():
    assert not host_build.clean(1, "") and not host_build.clean(-11, "") and not host_build.clean(2, WORDS)
