"""CPU: the two group kernels of the FLAC stage in the kernel census.

tests/test_kernel_census_cpu.py finds every `__global__` definition in csrc/*.cuh and csrc/*.hip and looks it up in its COVERAGE table;
a new kernel gets a reference test and then a line in that table.  flac_encode_group_kernel and flac_gather_group_kernel
(csrc/flac_kernels.cuh) have theirs, tests/test_gpu_flac_group.py: the single pushes and the reference encoder are the reference.  Their
two lines are ADDED TO THAT TABLE FROM HERE, when this module is imported, exactly as tests/test_level_group_census_cpu.py adds the
leveller's and the limiter's: pytest imports every test module before it runs the first test, so the census sees them whenever the suite
is collected, and checks them as it checks every other line."""
import test_kernel_census_cpu as census

try:                                       # the earlier add-ons' lines belong to the table this file checks as a whole, for as long as
    import test_limiter_census_cpu  # noqa: F401  they are registered from files of their own
except ImportError:
    pass
try:
    import test_stage_group_census_cpu  # noqa: F401
except ImportError:
    pass
try:
    import test_leveller_census_cpu  # noqa: F401
except ImportError:
    pass
try:
    import test_level_group_census_cpu  # noqa: F401
except ImportError:
    pass

TEST = "test_gpu_flac_group.py"
LINES = {
    "flac_encode_group_kernel": (TEST, TEST, "flac_kernels.cuh"),
    "flac_gather_group_kernel": (TEST, TEST, "flac_kernels.cuh"),
}
census.COVERAGE.update(LINES)


def test_the_group_kernels_are_in_the_census():
    ks = census.kernels()
    for name, line in LINES.items():
        assert ks.get(name) == line[2], (name, ks.get(name))
        assert census.COVERAGE.get(name) == line and name not in census.EXEMPT
    census.test_every_kernel_has_a_reference_test()                # the census's own check, over the table with the two lines in it
    for single in ("flac_encode_kernel", "flac_gather_kernel"):
        assert single in ks                                        # the single kernels keep their names beside the group kernels
