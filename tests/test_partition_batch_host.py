"""iqhip_partition_optimize_branch_batch without a device: the entry point exists and refuses a call without a group, a
task array or a result array before it touches HIP."""
import ctypes as C


def test_null_arguments_are_refused(pkg):
    lib = pkg.libiqhip()
    assert "iqhip_partition_optimize_branch_batch" in pkg.IQHIP_SYMBOLS
    task = (pkg.BranchTask * 1)(pkg.BranchTask(None, 0, 10, pkg.key_end(1), pkg.key_end(2), 0.1, 1e-6, 100.0, 1e-6))
    res = (pkg.BranchResult * 1)()
    assert lib.iqhip_partition_optimize_branch_batch(None, task, 1, res, None) == 2
    assert b"null group" in lib.iqhip_last_error()
    assert hasattr(pkg.PartitionGroup, "optimize_branch_batch")
