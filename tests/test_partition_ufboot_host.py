"""UFBoot on edge-linked partition models, the part that needs no device: the group entry points (include/iqhip.h "UFBoot on
edge-linked partition models") are exported, listed and bound, and each refuses a null group or null arguments with
IQHIP_ERR_INVALID before it touches a device."""
import ctypes as C

import numpy as np

IQHIP_ERR_INVALID = 2

NEW_SYMBOLS = ("iqhip_partition_ptnlh_reserve", "iqhip_partition_optimize_branch_batch_rows", "iqhip_partition_ptnlh_rell",
               "iqhip_partition_ufboot_init", "iqhip_partition_ufboot_update", "iqhip_partition_ufboot_fetch",
               "iqhip_debug_partition_ufboot_timing")


def test_new_symbols_exist(pkg):
    lib = pkg.libiqhip()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in pkg.IQHIP_SYMBOLS
        assert getattr(lib, s).argtypes is not None, s
    assert lib.iqhip_abi_version() == 2
    host = pkg.libiqhost()
    for s in ("iqhost_super_gen_boot_samples", "iqhost_super_nni_for_branch_rows", "iqhost_super_evaluate_nnis_list_rows"):
        assert hasattr(host, s), s
    for name in ("gen_boot_samples", "set_boot_samples", "ptnlh_reserve", "ptnlh_fetch", "ptnlh_rell", "ufboot_init",
                 "ufboot_update", "ufboot_state", "ufboot_timing", "save_current_tree", "save_nni_trees",
                 "ufboot_next_iteration", "summarize_bootstrap", "evaluate_nnis5_batch", "nni_for_branch"):
        assert callable(getattr(pkg.PhyloSuperTree, name)), name
    for name in ("ptnlh_reserve", "ptnlh_rell", "ufboot_init", "ufboot_update", "ufboot_state", "ufboot_timing"):
        assert callable(getattr(pkg.PartitionGroup, name)), name


def test_null_group_and_null_arguments_are_invalid(pkg):
    lib = pkg.libiqhip()
    out = np.zeros(8)
    dp = out.ctypes.data_as(C.POINTER(C.c_double))
    rows = np.zeros(2, dtype=np.int32)
    ip = rows.ctypes.data_as(C.POINTER(C.c_int32))
    ent = (pkg.UFBootTree * 1)(pkg.UFBootTree(0, 0, 1, -1.0, 0.5))
    task = (pkg.BranchTask * 1)(pkg.BranchTask(None, 0, 10, pkg.key_end(1), pkg.key_end(2), 0.1, 1e-6, 100.0, 1e-6))
    res = (pkg.BranchResult * 1)()
    calls = [lambda: lib.iqhip_partition_ptnlh_reserve(None, 2),
             lambda: lib.iqhip_partition_optimize_branch_batch_rows(None, task, 1, res, None, ip),
             lambda: lib.iqhip_partition_optimize_branch_batch_rows(None, None, 1, None, None, None),
             lambda: lib.iqhip_partition_ptnlh_rell(None, ip, 2, 1, dp),
             lambda: lib.iqhip_partition_ptnlh_rell(None, None, 2, 1, None),
             lambda: lib.iqhip_partition_ufboot_init(None, 4),
             lambda: lib.iqhip_partition_ufboot_update(None, ent, 1, 0.5, 0.0, None, None),
             lambda: lib.iqhip_partition_ufboot_update(None, None, 1, 0.5, 0.0, None, None),
             lambda: lib.iqhip_partition_ufboot_fetch(None, None, None, None, None),
             lambda: lib.iqhip_debug_partition_ufboot_timing(None, dp, None),
             lambda: lib.iqhip_debug_partition_ufboot_timing(None, None, None)]
    for k, call in enumerate(calls):
        assert call() == IQHIP_ERR_INVALID, k
        assert b"null group" in lib.iqhip_last_error(), (k, lib.iqhip_last_error())


def test_margin_seed_leaves_out_no_replicate_on_the_oracle_rows(pkg, synth, oracle):
    """The seed of tests/test_partition_ufboot_gpu.py::test_real_rows_against_the_numpy_product, screened here without a
    device: the current tree of the mixed group and its 10 nni5 neighbours from the oracle (lengths re-optimised jointly by
    the restatement of tests/partition_ref.py), the members' resamples drawn from the seed, and the margin scheme on numpy's
    product.  With this seed the reference computation alone leaves out no replicate, and by a wide margin."""
    import partition_ref as pr
    import partition_ufboot_ref as pu
    nwk, members = pr.mixed_group(synth, oracle)
    logl, Ls = pu.oracle_nni5_rows(oracle, nwk, members, pr.MIXED_RATES)
    assert len(logl) == 11 and all(L.shape == (11, d["pat"].shape[1]) for L, d in zip(Ls, members))
    for k in range(11):    # a row sums to its tree's log-likelihood
        assert abs(sum(float(L[k] @ d["freq"]) for L, d in zip(Ls, members)) - logl[k]) <= 1e-9 * abs(logl[k])
    assert (logl[1:] != logl[0]).all()
    ns = 257
    Ws = pu.member_samples(members, ns, pu.MARGIN_SEED)
    ids = np.arange(11, dtype=np.int64)
    rand = np.array([pkg.ufboot_rand(pu.TIE_SEED, k) for k in range(11)])
    want, counted, margins, bound = pu.margin_scheme(Ls, Ws, ids, logl, rand, ns)
    print("oracle rows, seed %d: left out %d of %d; smallest margin %.3e, largest bound %.3e"
          % (pu.MARGIN_SEED, (~counted).sum(), ns, margins.min(), bound.max()))
    assert counted.all()
    assert margins.min() > 1e3 * bound.max()
    assert len(set(want["boot_tree"].tolist())) > 1          # the replicates do disagree about the best tree
