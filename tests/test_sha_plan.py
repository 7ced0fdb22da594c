"""lcp2_witness_plan_rows_sha on the GPU: the plans of tests/sha_plan_cases.py through the library, with host lists and with lists in
HBM - equal to sha_plan_cases.plan_sha_model cell for cell on a matrix of arbitrary words; the Merkle tree equal word for word to what
lcp2_sha256_witness writes for the same leaves; without SHA jobs equal to lcp2_witness_plan_rows_u32; the refusals the device alone
can see; and 70 jobs in one level."""
import ctypes

import numpy as np
import pytest

import sha_plan_cases as cases
from rows_lib import INVALID, NW, DeviceMatrix, upload
from sha_plan_cases import BAD_FIRST, ENDS, LISTS, REASONS, REFUSAL_N, ROWS, SHA_FIRST, VALUE_REASON
from test_sha_rows import digest_src, make_jobs


def run_on_device(ctx, plan, start, device_lists=False):
    """(the matrix after the call, the Lcp2Error it raised or None)"""
    import eth_lc_plonky2_amd as m
    dm = DeviceMatrix(ctx, np.ascontiguousarray(start))
    ends = [getattr(plan, name) for name in ENDS]
    ptrs = [upload(ctx, getattr(plan, name)) for name in LISTS] if device_lists else []
    error = None
    try:
        if device_lists:
            ctx.witness_plan_rows_sha(*ptrs, *ends, dm.ptr, start.shape[0], start.shape[1], nsha=plan.sha_jobs.size, nu32=plan.u32_jobs.size,
                                      nrec=plan.rec_jobs.size, npos=plan.pos_jobs.size, nchains=plan.chain_ends.size, noperands=plan.operands.size)
        else:
            ctx.witness_plan_rows_sha(*[getattr(plan, name) for name in LISTS], *ends, dm.ptr, start.shape[0], start.shape[1])
    except m.Lcp2Error as e:
        error = e
    got = dm.read()
    dm.free()
    for ptr in ptrs:
        ctx.buffer_free(ptr)
    return got, error


@pytest.mark.gpu
@pytest.mark.parametrize("device_lists", [False, True])
@pytest.mark.parametrize("name", list(cases.CASES))
def test_cases_equal_the_model(gpu_ctx, name, device_lists):
    """(a)-(f) of sha_plan_cases: flat levels, the Merkle tree, four families, empty levels, non-canonical inputs, own-row operands"""
    plan, n, start, want = cases.case(name)
    got, error = run_on_device(gpu_ctx, plan, start, device_lists)
    assert error is None and (got == want).all()
    if not plan.u32_jobs.size + plan.rec_jobs.size + plan.pos_jobs.size:
        own = cases.owned_by_sha(plan, n)
        assert (got[~own] == start[~own]).all(), "a cell outside the 108 x 310 blocks was touched"


@pytest.mark.gpu
def test_merkle_tree_equals_sha256_witness(gpu_ctx):
    """the reference is the existing call: the same tree as lcp2_sha256_witness jobs, the leaves as words_in - the SHA rows agree word
    for word, the returned digests are the digest cells, the root is hashlib's"""
    plan, n, start, want = cases.case("merkle")
    leaves, rows, root = cases.merkle_parts()
    items = [(rows[j], list(range(16 * j, 16 * j + 16))) for j in range(4)]
    items += [(rows[4 + j], [digest_src(2 * j + side, i) for side in (0, 1) for i in range(8)]) for j in range(2)]
    items += [(rows[6], [digest_src(4 + side, i) for side in (0, 1) for i in range(8)])]
    dm = DeviceMatrix(gpu_ctx, np.ascontiguousarray(start))
    digests = gpu_ctx.sha256_witness(make_jobs(items), [0, 4, 6, 7], leaves.astype(np.uint32).ravel(), dm.ptr, n)
    reference = dm.read()
    dm.free()
    got, error = run_on_device(gpu_ctx, plan, start, device_lists=True)
    own = cases.owned_by_sha(plan, n)
    assert error is None and (got[own] == reference[own]).all() and (got == reference).all()
    for j in range(7):
        assert cases.digest_of(got, rows[j]) == digests[j].tolist(), j
    assert cases.digest_of(got, rows[6]) == root


@pytest.mark.gpu
def test_without_sha_jobs_it_is_witness_plan_rows_u32(gpu_ctx):
    from test_u32_plan_emu import mixed_levels
    plan = cases.sp().pack_sha_plan([([],) + tuple(level) for level in mixed_levels()])
    start = cases.pattern(64, 4)
    dm = DeviceMatrix(gpu_ctx, start)
    gpu_ctx.witness_plan_rows_u32(*[getattr(plan, name) for name in LISTS[1:]], *[getattr(plan, name) for name in ENDS[1:]], dm.ptr, NW, 64)
    reference = dm.read()
    dm.free()
    assert not (reference == start).all()
    for device_lists in (False, True):
        got, error = run_on_device(gpu_ctx, plan, start, device_lists)
        assert error is None and (got == reference).all()


@pytest.mark.gpu
def test_refusals_found_on_the_device(gpu_ctx):
    """a cell holding 2^32, from host and device lists, and a CELL row out of range in a device list: the refused job writes nothing,
    its level and the earlier ones are written, later levels are not in any family, the job is named with its reason.  A refused host
    list writes nothing.  The four families in one level: rec is named before SHA before u32 before poseidon"""
    from test_u32_plan_emu import BAD_ROW, index_of, index_of_rec
    from test_u32_plan_emu import reason_cases as u32_reason_cases
    s = cases.sp()
    start = cases.refusal_start()
    for code, by_cell, kinds in ((VALUE_REASON, True, (False, True)), (5, False, (True,))):
        plan, at, kept = cases.refused_plan(code, by_cell=by_cell)
        want = cases.plan_sha_model(start, kept)
        for device_lists in kinds:
            got, error = run_on_device(gpu_ctx, plan, start, device_lists)
            assert error is not None and error.status == INVALID and "plan rows: sha job %d: %s" % (at, REASONS[code]) in str(error), str(error)
            assert "found on the device" in str(error)
            assert (got == want).all() and not got[:, BAD_FIRST:].any() and not got[:, SHA_FIRST[2]:].any() and not got[:, [7, 43, 52]].any()
            assert got[:, SHA_FIRST[0]:SHA_FIRST[2]].any(axis=0).all() and got[:, [3, 4, 41, 51]].any(axis=0).all()
    plan, at, _ = cases.refused_plan(5)
    got, error = run_on_device(gpu_ctx, plan, start)
    assert error is not None and error.status == INVALID and "plan rows: sha job %d: cell operand row out of range" % at in str(error)
    assert "found on the device" not in str(error) and (got == start).all(), "a refused host list wrote something"
    bad_sha, bad_u32 = cases.reason_cases(by_cell=True)[VALUE_REASON][0], u32_reason_cases(by_cell=True)[4][0]
    for bad_rec, family in ((True, "rec"), (False, "sha")):
        levels, kept = cases.refusal_levels(bad_sha, bad_u32=bad_u32, bad_rec=bad_rec, bad_swap=True)
        plan = s.pack_sha_plan(levels)
        assert index_of(plan, BAD_ROW) >= 0
        text = {"rec": "plan rows: rec job %d: random-access index" % index_of_rec(plan, 30) if bad_rec else "",
                "sha": "plan rows: sha job %d: operand value of 2^32 or more" % cases.index_of_sha(plan, BAD_FIRST)}[family]
        for device_lists in (False, True):
            got, error = run_on_device(gpu_ctx, plan, start, device_lists)
            assert error is not None and error.status == INVALID and text in str(error), str(error)
            assert (got == cases.plan_sha_model(start, s.pack_sha_plan(kept))).all(), (family, device_lists)
    good = s.pack_sha_plan(cases.refusal_levels()[0])   # the context still works
    got, error = run_on_device(gpu_ctx, good, start)
    assert error is None and (got == cases.plan_sha_model(start, good)).all()


@pytest.mark.gpu
def test_seventy_jobs_in_one_level(gpu_ctx):
    plan, n, start, want = cases.case("wide")
    assert plan.sha_jobs.size == 70 and plan.sha_level_ends.tolist() == [70]
    got, error = run_on_device(gpu_ctx, plan, start, device_lists=True)
    assert error is None and (got == want).all()


@pytest.mark.gpu
def test_argument_checks(gpu_ctx):
    import eth_lc_plonky2_amd as m
    s = cases.sp()
    lib, n = gpu_ctx.lib, REFUSAL_N
    good = s.pack_sha_plan(cases.refusal_levels()[0])
    start = cases.refusal_start()
    dm = DeviceMatrix(gpu_ctx, start)
    wp, h = ctypes.c_void_p(dm.ptr), gpu_ctx.handle
    call = lambda p, mem=m.MEM_HOST, w=wp, ncols=NW: lib.lcp2_witness_plan_rows_sha(h, ctypes.byref(p) if p is not None else None, mem, w, ncols, n)   # noqa: E731
    p, keep = cases.plan_struct(m, good)
    assert call(None) == INVALID and call(p, w=None) == INVALID and call(p, mem=2) == INVALID and call(p, ncols=134) == INVALID
    assert b"135 columns" in lib.lcp2_last_error(h)
    for field in ("sha_jobs", "sha_level_ends"):
        p, keep = cases.plan_struct(m, good)
        setattr(p, field, None)
        assert call(p) == INVALID and call(p, mem=m.MEM_DEVICE) == INVALID and b"null" in lib.lcp2_last_error(h), field
    for values in ([1, 3, 2], [1, 0, 3], [1, 2, 2]):
        broken = type(good)(**vars(good))
        broken.sha_level_ends = np.array(values, dtype=np.uint32)
        p, keep = cases.plan_struct(m, broken)
        assert call(p) == INVALID and b"sha_level_ends" in lib.lcp2_last_error(h), values
    p, keep = cases.plan_struct(m, good, {"nsha": 1 << 32})
    assert call(p, mem=m.MEM_DEVICE) == INVALID and b"2^32 - 1" in lib.lcp2_last_error(h)
    p, keep = cases.plan_struct(m, good, {"nlevels": 0})
    assert call(p) == INVALID
    p, keep = cases.plan_struct(m, s.pack_sha_plan([([], [], [], []), ([], [], [], [[]])]))   # empty levels, an empty chain: nothing to do
    assert call(p) == 0 and call(p, mem=m.MEM_DEVICE) == 0
    p, keep = cases.plan_struct(m, good, {"nsha": 0, "nu32": 0, "nrec": 0, "npos": 0})
    assert call(p) == 0
    assert (dm.read() == start).all()
    p, keep = cases.plan_struct(m, good)
    assert call(p) == 0 and (dm.read() == cases.plan_sha_model(start, good)).all()
    dm.free()
