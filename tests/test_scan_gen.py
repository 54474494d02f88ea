"""TorchOusterSim.scans(k0, n), the batched generator bench.py builds its steps with, gives
scan(k)'s points bit for bit: same float32 words, same offsets, same origins, whatever the chunk
size -- so a bench step holds the same cloud whichever of the two made it."""
import numpy as np
import pytest


def _check(device, beams, hz, k0, n, chunk):
    import torch
    from tsdf_map.scan_gen import TorchOusterSim
    sim = TorchOusterSim(device, beams=beams, hz=hz)
    ref = [sim.scan(k) for k in range(k0, k0 + n)]
    x, offs, org = sim.scans(k0, n, chunk=chunk)
    assert x.dtype == torch.float32 and x.is_contiguous() and offs.dtype == np.uint64
    assert offs.tolist() == np.concatenate([[0], np.cumsum([p.shape[0] for p, _ in ref])]).tolist()
    assert org.dtype == np.float64 and np.array_equal(org, np.stack([o for _, o in ref]))
    want = torch.cat([p for p, _ in ref])
    assert x.shape == want.shape and x.shape[0] > 0
    assert bool((x.view(torch.int32) == want.view(torch.int32)).all())
    # the seeded noise repeats: the same arguments give the same cloud
    assert bool((sim.scans(k0, n, chunk=chunk)[0].view(torch.int32) == x.view(torch.int32)).all())


@pytest.mark.parametrize("beams,hz,k0,n,chunk", [("os1_128_1024", 10.0, 37, 5, 2),
                                                 ("os1_128_2048", 20.0, 0, 3, 64)])
def test_batched_scans_equal_single_scans_cpu(beams, hz, k0, n, chunk):
    import torch
    _check(torch.device("cpu"), beams, hz, k0, n, chunk)


@pytest.mark.gpu
@pytest.mark.parametrize("beams,hz,k0,n,chunk", [("os1_128_1024", 10.0, 1000, 5, 2),
                                                 ("os1_128_1024", 10.0, 64, 4, 64),
                                                 ("os1_128_2048", 20.0, 7, 3, 3)])
def test_batched_scans_equal_single_scans_gpu(beams, hz, k0, n, chunk):
    import torch
    _check(torch.device("cuda", 0), beams, hz, k0, n, chunk)
