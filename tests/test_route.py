"""Where a batch of rounds runs (pcx_batched_route, pyconsensus_amd.batched.route) and what the
workgroup-per-round kernel asks of LDS (pcx_medium_lds_bytes).  Pure functions of their arguments:
no GPU."""
import pytest

ALGS = {"PCA": 0, "absolute": 1, "big-five": 2, "fixed-variance": 3, "cokurtosis": 4, "k-means": 5,
        "hierarchical": 6, "clusterfeck": 7}
PLAIN = ("PCA", "absolute", "big-five", "fixed-variance", "cokurtosis")
WAVE, WORKGROUP, SCHEDULER = 0, 1, 2


def _lib():
    from pyconsensus_amd import _lib

    return _lib.lib()


def test_route_table():
    from pyconsensus_amd.batched import kmeans_k, route

    h = _lib()
    for N, E in ((50, 20), (64, 32)):
        for name, alg in ALGS.items():
            assert h.pcx_batched_route(N, E, alg, kmeans_k(N)) == WAVE, (N, E, name)
            assert route(N, E, name) == "wave"
    for N, E in ((65, 2), (3, 40), (100, 50), (256, 64)):
        for name in PLAIN + ("hierarchical", "clusterfeck", "k-means"):
            k = kmeans_k(N)
            assert k <= 16
            assert h.pcx_batched_route(N, E, ALGS[name], k) == WORKGROUP, (N, E, name)
            assert route(N, E, name) == "workgroup"
    assert h.pcx_batched_route(256, 64, ALGS["k-means"], 16) == WORKGROUP
    assert h.pcx_batched_route(256, 64, ALGS["k-means"], 1) == WORKGROUP
    for N, E in ((257, 10), (10, 65)):
        for name, alg in ALGS.items():
            assert h.pcx_batched_route(N, E, alg, kmeans_k(N)) == SCHEDULER, (N, E, name)
            assert route(N, E, name) == "scheduler"
    assert h.pcx_batched_route(100, 50, ALGS["k-means"], 17) == SCHEDULER
    assert route(100, 50, "k-means", kmeans_k=17) == "scheduler"
    assert route(100, 50, "k-means", kmeans_k=16) == "workgroup"
    # kmeans_k matters for k-means only
    assert h.pcx_batched_route(100, 50, ALGS["PCA"], 17) == WORKGROUP
    assert h.pcx_batched_route(100, 50, ALGS["clusterfeck"], 0) == WORKGROUP


def test_route_refusals():
    from pyconsensus_amd.batched import route

    h = _lib()
    assert h.pcx_batched_route(50, 20, 8, 8) == -1
    assert h.pcx_batched_route(50, 20, -1, 8) == -1
    assert h.pcx_batched_route(0, 20, 0, 8) == -1
    assert h.pcx_batched_route(50, 0, 0, 8) == -1
    # k-means code books the batched entry refuses: none, more than reporters, more than 8 in a wave
    assert h.pcx_batched_route(50, 20, ALGS["k-means"], 0) == -1
    assert h.pcx_batched_route(50, 20, ALGS["k-means"], 9) == -1
    assert h.pcx_batched_route(3, 40, ALGS["k-means"], 4) == -1
    with pytest.raises(ValueError):
        route(0, 5)
    with pytest.raises(NotImplementedError):
        route(50, 20, "no-such")


def test_route_ignores_the_scheduler_override(monkeypatch):
    monkeypatch.setenv("PCX_NO_MEDIUM", "1")
    assert _lib().pcx_batched_route(100, 50, ALGS["clusterfeck"], 10) == WORKGROUP


# ---- the workgroup kernel's dynamic LDS: the layout before the clusterings, restated
def _pow2(N):
    p = 2
    while p < N:
        p <<= 1
    return p


def _work_before(N, E, jacobi):
    E4 = 0 if E == 1 else E & ~3
    pn = _pow2(N)
    mt = (2 if jacobi else 1) * E * (E + 1)
    wq = 4 * (2 * N + 2 * pn + pn // 2)
    vb = (N >> 2) * E4 + (E - E4) * N
    return max(mt, wq, vb)


def _lds_bytes_before(N, E, alg):
    """medium_lds_bytes before the clusterings: the work region, 11 N-vectors, 22 E-vectors,
    two flag bits per element in 32-bit words, 16 bytes of slack."""
    return (_work_before(N, E, alg in (2, 3)) + 11 * N + 22 * E) * 8 + ((N * E + 15) >> 4) * 4 + 16


def test_medium_lds_fits_a_workgroup():
    h = _lib()
    assert _lds_bytes_before(256, 64, 0) == 74768
    for name, alg in ALGS.items():
        for N in range(1, 257):
            for E in range(1, 65):
                got = h.pcx_medium_lds_bytes(N, E, alg)
                assert 0 < got <= 160 * 1024, (name, N, E, got)
                if name in PLAIN:
                    assert got == _lds_bytes_before(N, E, alg), (name, N, E, got)
                else:  # never less than the PCA steps they run first
                    assert got >= _lds_bytes_before(N, E, 0), (name, N, E, got)
    assert h.pcx_medium_lds_bytes(257, 10, 0) == 0 and h.pcx_medium_lds_bytes(10, 65, 0) == 0
    assert h.pcx_medium_lds_bytes(100, 50, 8) == 0
