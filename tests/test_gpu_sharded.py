"""GPU tests of the row-sharded path: two ranks share the one GPU, slices are exchanged through host memory
(gloo), and the result must equal the single-rank run bit for bit; plus the RCCL self-test."""
import pytest

from test_dist_gloo import launch

pytestmark = pytest.mark.gpu


def test_rccl_selftest(qn):
    qn.default_context().comm_selftest()


def test_two_ranks_on_one_gpu_equal_single_rank_bitwise(tmp_path):
    res = launch("gpu", tmp_path, timeout=600)
    assert len(res) == 2
    for r in res:
        assert r["iters"] == 25
        assert r["trace_equal"] and r["x_equal"] and r["h_equal"], r
        assert r["objective_rows_ok"] and r["eval_equal"] and r["dfp_bt_equal"], r
        assert r["lse_eval_close"] and r["lse_dfp_close"], r


def _device_count():
    # (in a child process: importing torch HERE, after libqn_hip.so has initialised HIP and loaded RCCL in this process, ends in a double free
    # at interpreter exit when this file is run by itself -- two runtimes' teardown orders; with `-m gpu` conftest.py imports torch first)
    import subprocess
    import sys
    out = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.device_count())"], capture_output=True, text=True, timeout=600)
    try:
        return int(out.stdout.strip().splitlines()[-1])
    except (ValueError, IndexError):
        return 0


def _check_sharded_symmetric(res, nproc):
    """Row-sharded runs stream the symmetric half too (circulant windows over the block-rows, qn_sym.hip.h): two / three ranks
    on the one GPU against the single-rank run -- same line-search decisions, iterates to the parity tolerance, identical bits
    on every rank, half the matrix bytes per pass, and the getters / the row kernels see a whole matrix again afterwards."""
    assert len(res) == nproc
    for r in res:  # nothing is left behind: the owners' count and bytes are back where they were once every handle is closed
        assert r["live_allocations"][0] == r["live_allocations"][1], (r["rank"], r["live_allocations"])
    for r in res:
        for case in r["cases"]:
            n = case["n"]
            nb = (n + 127) // 128
            for m in ("bfgs", "dfp"):
                assert case[m + "_close"] and case[m + "_h_symmetric"] and case[m + "_h_close"], (r["rank"], case)
                assert case[m + "_again_close"] and case[m + "_rows_close"], (r["rank"], case)
                p_sh, p_1 = case[m + "_path"]
                assert p_sh & 1 and p_sh & 2, p_sh   # fused, symmetric storage
                # whole 128-blocks (n = n_pad): the second-generation structure (qn_sym2sh.hip.h); padded n: rounds 1-3's kernels
                assert bool(p_sh & 16) == (n % 128 == 0), (n, p_sh)
                assert case[m + "_again_path"] & 2 and not case[m + "_rows_path"] & 2
                b_sh, b_1 = case[m + "_bytes"]
                assert abs(nproc * b_sh - nb * (nb + 1) // 2 * 131072) <= nproc * (nb // nproc) * 131072  # balanced to one tile per block-row
            assert case["gen1_close"] and case["gen1_path"] & 2 and not case["gen1_path"] & 16, case  # rounds 1-3's kernels, still reachable
    for r in res:  # the generic path's H pass on the sharded tiles (flag 4), quadratic and log-sum-exp objectives
        for case in r["cases"]:
            assert case["generic_close"] and case["generic_path"][0] & 4 and not case["generic_path"][0] & 1, case
            if "lse_close" in case:
                # the log-sum-exp objective, rows of A sharded: the second-generation structure (round 5) on the ranks and on one rank --
                # one scalar collective per evaluation, two n-vector collectives per iteration (+ the run's opening pair) --, the generic
                # path still reachable, and the stream-ordered exchange (pipelined) bit for bit the synchronous pump
                assert case["lse_close"] and case["lse_path"][0] & 16 and case["lse_path"][0] & 2 and case["lse_path"][1] & 16, case
                ev, xs_, xv, it = case["lse_xchg"]
                assert xs_ == ev and xv == 2 * it + 2, case["lse_xchg"]
                assert case["lse_generic_close"] and case["lse_generic_path"] & 4 and not case["lse_generic_path"] & 16, case
                if "lse_pipelined_equal" in case:
                    assert case["lse_pipelined_equal"] and case["lse_pipelined_path"] & 8 and case["lse_pipelined_path"] & 16, case
            if "mt_cases_ok" in case:  # cases 2, 3 and 4 really occurred on the sharded tiles, and matched the single-rank run
                assert case["mt_cases_ok"] and min(case["mt_digits"][1:]) >= 3, case
    nbs = {case["n"]: (case["n"] + 127) // 128 for case in res[0]["cases"]}
    for i, case in enumerate(res[0]["cases"]):
        assert sum(r["cases"][i]["generic_bytes"] for r in res) == nbs[case["n"]] * (nbs[case["n"]] + 1) // 2 * 131072
    for r in res:  # stream-ordered host exchange: pipelined (flag 8), far fewer synchronisations, the same bits
        for case in r["cases"]:
            assert case["pipelined_equal"] and case["rows_pipelined_equal"] and case["allreduce_ok"], case
            assert not case["pipelined_path"][0] & 8 and case["pipelined_path"][1] & 8 and case["pipelined_path"][1] & 2
            assert not case["rows_pipelined_path"][0] & 8 and case["rows_pipelined_path"][1] & 8
            assert case["pipelined_syncs"][1] * 4 < case["pipelined_syncs"][0]  # (the control-block reads; the exchanges' own waits are not even counted)
            if "trial_vector" in case:  # (round 6) the trial's partial vector on the scalar exchange: the default exchange's bits, pump and pipelined
                for tv in case["trial_vector"]:
                    assert tv["equal"], case
                tv0 = case["trial_vector"][0]
                if case["n"] % 128 == 0 and tv0["path"] & 16 and not tv0["path"] & 8:  # second-generation structure, synchronous pump: exact counts
                    dv, ds, dit = case["default_xchg"]
                    assert dv == 2 * dit + 2 and tv0["xchg"] == [tv0["iters"] + 1, tv0["evals"]], case
                if len(case["trial_vector"]) > 1:  # stream-ordered host exchange: pipelined
                    tv1 = case["trial_vector"][1]
                    assert tv1["path"] & 8 and tv1["syncs"] * 4 < tv0["syncs"], case
                    if case["n"] % 128 == 0 and tv1["path"] & 16:
                        assert tv1["xchg"][0] < case["default_xchg"][0] or tv1["iters"] == 0, case
            if "bt_pipelined_equal" in case:  # backtracking with a varying number of evaluations per iteration: sized pattern, roll-over
                assert case["bt_pipelined_equal"] and case["bt_evals"][0] == case["bt_evals"][1], case
                assert not case["bt_paths"][0] & 8 and case["bt_paths"][1] & 8
                assert case["bt_evals_per_iteration_max"] >= 3  # (the workload does search: more evaluations than the two slots a period starts with)
                if case["n"] % 128 == 0:  # second-generation structure: the synchronous pump enqueues exactly one scalar exchange per evaluation
                    assert case["bt_xchg"][0][0] == case["bt_evals"][0] and case["bt_xchg"][1][0] >= case["bt_evals"][1], case
    for case_i in range(len(res[0]["cases"])):
        n_i = res[0]["cases"][case_i]["n"]
        nb = (n_i + 127) // 128
        # the ranks' tiles together are the half matrix exactly: every pair of block-rows once
        assert sum(r["cases"][case_i]["gen1_bytes"] for r in res) == nb * (nb + 1) // 2 * 131072
        for m in ("bfgs", "dfp"):
            # (the second-generation kernels stream a diagonal tile as its upper triangle: 73 728 of its 131 072 bytes)
            diag_tile = 73728 if n_i % 128 == 0 else 131072
            assert sum(r["cases"][case_i][m + "_bytes"][0] for r in res) == nb * (nb - 1) // 2 * 131072 + nb * diag_tile
            assert len({tuple(r["cases"][case_i][m + "_x_hex"]) for r in res}) == 1  # replicated vector work: same bits everywhere
            assert len({tuple(r["cases"][case_i][m + "_h_hex"]) for r in res}) == 1
        assert len({tuple(r["cases"][case_i]["allreduce_x_hex"]) for r in res}) == 1  # all-reduce mode: the same bits on every rank too


@pytest.mark.parametrize("nproc", [2, 3])
def test_row_sharded_symmetric_storage(tmp_path, nproc):
    _check_sharded_symmetric(launch("gpu_sym", tmp_path, nproc=nproc, timeout=900), nproc)


@pytest.mark.parametrize("nproc", [2, 4, 8])
def test_row_sharded_symmetric_storage_over_rccl(tmp_path, nproc):
    """The same checks with one GPU per rank and the real RCCL exchange (all-gathers, single and grouped, and ncclAllReduce),
    pipelined against synchronous: runs at 2, 4 and 8 ranks on the first box that has that many GPUs (none was available to
    this build in rounds 1-3; the partitions themselves are rehearsed on one GPU in tests/test_gpu_partitions.py)."""
    if _device_count() < nproc:
        pytest.skip("needs %d GPUs: the RCCL exchange between devices" % nproc)
    _check_sharded_symmetric(launch("gpu_sym", tmp_path, nproc=nproc, timeout=900, extra_env={"QN_TEST_EXCHANGE": "rccl"}), nproc)
