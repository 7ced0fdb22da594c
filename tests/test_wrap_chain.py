"""Shrinking the light-client proof by recursion (plonky2's test_size_optimized_recursion): LC step -> wrap (rate_bits 7, cap 4,
12 queries, 16 PoW bits) -> wrap (rate_bits 8, cap 0, 10 queries, 20 PoW bits), through liblcp2_host.so and through
examples/lc_prover --shrink."""
import re

import numpy as np
import pytest

import cpp_build

WRAP_1 = (7, 4, 16, 12)
WRAP_2 = (8, 0, 20, 10)


@pytest.mark.gpu
def test_wrap_chain_in_process(gpu_ctx):
    """each step verifies, carries the LC step's public inputs and is smaller than the one before it; a wrap of a tampered inner
    proof is LCP2_E_UNSAT"""
    import eth_lc_plonky2_amd as m
    from eth_lc_plonky2_amd import light_client as lc
    prev, cur = lc.reference_updates()
    step = lc.LightClientStep(gpu_ctx, prev, cur)
    proof, pis = step.prove()

    w1 = lc.WrapStep(gpu_ctx, step, *WRAP_1)
    assert w1.info.inner_degree_bits == 19 and w1.info.num_public_inputs == 16
    p1, pis1 = w1.prove(proof, pis)
    w1.verify(p1, pis1)
    assert (pis1 == step.expected_public_inputs).all()
    bad = proof.copy()
    bad[len(bad) // 3] = np.uint64((int(bad[len(bad) // 3]) + 1) % m.GOLDILOCKS_P)
    with pytest.raises(m.Lcp2Error) as e:
        w1.prove(bad, pis)
    assert e.value.status == -5  # LCP2_E_UNSAT

    w2 = lc.WrapStep(gpu_ctx, w1, *WRAP_2)
    p2, pis2 = w2.prove(p1, pis1)
    w2.verify(p2, pis2)
    assert (pis2 == step.expected_public_inputs).all()
    bad = p2.copy()
    bad[len(bad) // 2] ^= np.uint64(1)
    with pytest.raises(m.ProofRejected):
        w2.verify(bad, pis2)
    assert p1.size < proof.size and p2.size < proof.size
    for s in (w2, w1, step):
        s.close()


@pytest.mark.gpu
def test_lc_prover_shrink(tmp_path):
    """examples/lc_prover --shrink: both wraps verify and the final proof has fewer bytes than the light-client step's"""
    import eth_lc_plonky2_amd as m
    prev, cur = m.light_client.reference_updates()
    files = []
    for name, text in (("prev.json", prev), ("cur.json", cur)):
        f = tmp_path / name
        f.write_text(text)
        files.append(str(f))
    r = cpp_build.run_example(files + ["--shrink"], timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    sizes = {int(k): int(b) for k, b in re.findall(r"shrink step (\d) .*?(\d+) bytes", r.stdout)}
    assert sorted(sizes) == [0, 1, 2], r.stdout
    assert sizes[2] < sizes[0] and sizes[1] < sizes[0], sizes
    assert r.stdout.count("verified") >= 2
