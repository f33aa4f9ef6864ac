"""tests/concurrent_jobs.py on the CPU: the module imports without a device, every job's expected value comes out of the references alone, and a
case job's comparison tells the reference's bytes from anything else."""
import time

import numpy as np
import pytest

import concurrent_jobs as CJ


def test_the_table_covers_the_four_roles():
    names = [j.name for j in CJ.jobs()]
    assert len(set(names)) == len(names)
    for role in CJ.ROLES:
        assert len(CJ.by_role(role)) >= 5, role


@pytest.mark.parametrize("job", CJ.jobs(), ids=lambda j: repr(j))
def test_expected_value_from_the_references_alone(job):
    t0 = time.time()
    a = job.expected()
    assert a is not None and job.expected() is a                 # computed once per process
    print("%r: %.2f s" % (job, time.time() - t0))


def test_case_comparison_sees_the_fill_the_decoy_and_a_flipped_bit():
    case = next(j for j in CJ.jobs() if j.name.startswith("kf_redundancy")).expected()
    real = {k: np.full(n, CJ.FILL, np.uint8) for k, n in case.outputs.items()}
    decoy = {k: v.copy() for k, v in real.items()}
    for k, segs in case.expect.items():
        for off, r, d in segs:
            real[k][off:off + CJ._raw(r).nbytes] = CJ._raw(r)
            decoy[k][off:off + CJ._raw(d).nbytes] = CJ._raw(d)
    assert CJ.case_mismatch(case, real) is None
    assert "other bytes" in CJ.case_mismatch(case, decoy)
    assert "the fill" in CJ.case_mismatch(case, {k: np.full(n, CJ.FILL, np.uint8) for k, n in case.outputs.items()})
    k = next(iter(case.expect))
    real[k][0] ^= 1
    assert k in CJ.case_mismatch(case, real)
