"""CPU tests (no GPU): the five workspace queries of the forward-dynamics family, pinned byte for byte to the values recorded in
tests/golden/dynamics_workspace_bytes.json (tools/record_dynamics_workspace_bytes.py wrote it; it is recorded once and not
regenerated from the build under test), and the nesting the layouts promise.  A workspace a caller sized with an earlier build
must still fit.  Nothing here touches a device."""
import json

import pytest

from _cabi import CHUNKED, CHUNKS, GOLDEN_FILE, INTEGRATOR_CODES as INTEGRATORS, SAMPLES, SWEPT, measure


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN_FILE) as f:
        return json.load(f)


@pytest.mark.parametrize("name", CHUNKED)
def test_queries_return_the_recorded_bytes(name, golden):
    got = measure(name)
    assert sorted(got) == sorted(golden[name])
    for query, sizes in got.items():
        assert len(sizes) == (len(CHUNKS) if query in ("forward", "derivatives", "vjp") else len(CHUNKS) * len(SAMPLES) * len(INTEGRATORS))
        assert sizes == golden[name][query], query
        assert all(s > 0 and s % 256 == 0 for s in sizes.values()), query


@pytest.mark.parametrize("name", CHUNKED)
def test_layouts_nest(name):
    got = measure(name)
    for chunk in CHUNKS:
        k = str(chunk)
        assert got["derivatives"][k] >= got["forward"][k]
        assert got["vjp"][k] >= got["derivatives"][k]
        for integrator in INTEGRATORS:
            for N in SAMPLES:
                key = "%d/%d/%d" % (integrator, N, chunk)
                assert got["adjoint"][key] >= got["vjp"][k]
                assert got["rollout"][key] >= got["forward"][k]


@pytest.mark.parametrize("name", SWEPT)
def test_swept_chains_need_none(name):
    for sizes in measure(name).values():
        assert all(s == 0 for s in sizes.values())
