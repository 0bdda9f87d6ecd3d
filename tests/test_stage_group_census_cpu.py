"""CPU: the two group kernels of the output stages in the kernel census.

tests/test_kernel_census_cpu.py finds every `__global__` definition in csrc/*.cuh and csrc/*.hip and looks it up in its COVERAGE table;
a new kernel gets a reference test and then a line in that table.  audio_out_group_kernel (csrc/audio_kernels.cuh) and tsm_group_kernel
(csrc/tsm_kernels.cuh) have theirs, tests/test_gpu_stage_group.py: the single pushes, checked against their own references, are the
reference.  Their two lines are ADDED TO THAT TABLE FROM HERE, when this module is imported, exactly as tests/test_limiter_census_cpu.py
adds the limiter's: pytest imports every test module before it runs the first test, so the census sees them whenever the suite is
collected, and checks them as it checks every other line."""
import test_kernel_census_cpu as census

try:                                       # the limiter's lines belong to the table this file checks as a whole, for as long as
    import test_limiter_census_cpu  # noqa: F401  they are registered from a file of their own
except ImportError:
    pass

LINES = {
    "audio_out_group_kernel": ("test_gpu_stage_group.py", "test_gpu_stage_group.py", "audio_kernels.cuh"),
    "tsm_group_kernel": ("test_gpu_stage_group.py", "test_gpu_stage_group.py", "tsm_kernels.cuh"),
}
census.COVERAGE.update(LINES)


def test_the_group_kernels_are_in_the_census():
    ks = census.kernels()
    for name, line in LINES.items():
        assert ks.get(name) == line[2], (name, ks.get(name))
        assert census.COVERAGE.get(name) == line and name not in census.EXEMPT
    census.test_every_kernel_has_a_reference_test()                # the census's own check, over the table with the two lines in it
