"""CPU: the leveller's three kernels in the kernel census.

tests/test_kernel_census_cpu.py finds every `__global__` definition in csrc/*.cuh and csrc/*.hip and looks it up in its COVERAGE table;
a new kernel gets a reference test and then a line in that table.  The leveller's kernels (csrc/level_kernels.cuh) have their reference
test, tests/test_gpu_leveller.py.  Their lines are ADDED TO THAT TABLE FROM HERE, when this module is imported: pytest imports every
test module before it runs the first test, so the census sees them whenever the suite (or both files) is collected, and checks them as
it checks every other line -- the test exists, is a GPU test, and names the kernels' header.  Run on its own, the census file reports
the kernels as missing; the lines move into its own table with the next change to it, and this file then goes."""
import test_kernel_census_cpu as census

LINES = {
    "level_target_kernel": ("test_gpu_leveller.py", "test_gpu_leveller.py", "level_kernels.cuh"),
    "level_apply_kernel": ("test_gpu_leveller.py", "test_gpu_leveller.py", "level_kernels.cuh"),
    "level_stats_kernel": ("test_gpu_leveller.py", "test_gpu_leveller.py", "level_kernels.cuh"),
}
census.COVERAGE.update(LINES)


def test_the_leveller_kernels_are_in_the_census():
    ks = census.kernels()
    for name, line in LINES.items():
        assert ks.get(name) == "level_kernels.cuh", (name, ks.get(name))
        assert census.COVERAGE.get(name) == line and name not in census.EXEMPT
    census.test_every_kernel_has_a_reference_test()                # the census's own check, over the table with the lines in it
    assert ks.get("loud_push_kernel") == "loud_kernels.cuh"        # the meter's kernels stay where they were: the leveller launches them
