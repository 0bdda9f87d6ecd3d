"""CPU: the group kernel of the segment join in the kernel census.

tests/test_kernel_census_cpu.py finds every `__global__` definition in csrc/*.cuh and csrc/*.hip and looks it up in its COVERAGE table;
a new kernel gets a reference test and then a line in that table.  join_group_kernel (csrc/join_kernels.cuh) has its own,
tests/test_gpu_join_group.py: the single pushes and tests/_join_ref.py are the reference.  Its line is ADDED TO THAT TABLE FROM HERE,
when this module is imported, exactly as tests/test_flac_group_census_cpu.py adds the FLAC stage's: pytest imports every test module
before it runs the first test, so the census sees it whenever the suite is collected, and checks it as it checks every other line."""
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
try:
    import test_flac_group_census_cpu  # noqa: F401
except ImportError:
    pass

TEST = "test_gpu_join_group.py"
LINES = {
    "join_group_kernel": (TEST, TEST, "join_kernels.cuh"),
}
census.COVERAGE.update(LINES)


def test_the_group_kernel_is_in_the_census():
    ks = census.kernels()
    for name, line in LINES.items():
        assert ks.get(name) == line[2], (name, ks.get(name))
        assert census.COVERAGE.get(name) == line and name not in census.EXEMPT
    census.test_every_kernel_has_a_reference_test()                # the census's own check, over the table with the line in it
    assert ks.get("join_kernel") == "join_kernels.cuh"             # the single kernel keeps its name beside the group kernel
