"""The device-salt registry of ``parallel/rng.py``: the dropout launchers read
``device_salt_ptr()`` at launch time; the tensor is held weakly, so the
address reads 0 again as soon as its owner lets go of it."""
import gc

import torch

from fleetx_amd.parallel import rng


def test_device_salt_registry():
    rng.set_device_salt(None)
    assert rng.device_salt_ptr() == 0
    a = torch.zeros(1, dtype=torch.int64)
    b = torch.zeros(1, dtype=torch.int64)
    try:
        rng.set_device_salt(a)
        assert rng.device_salt_ptr() == a.data_ptr() != 0
        rng.set_device_salt(b)  # a second set replaces the first
        assert rng.device_salt_ptr() == b.data_ptr() != a.data_ptr()
        del a
        gc.collect()
        assert rng.device_salt_ptr() == b.data_ptr()
        del b
        gc.collect()
        assert rng.device_salt_ptr() == 0  # no owner left: eager keys again
        rng.set_device_salt(torch.zeros(1, dtype=torch.int64))  # never owned by anyone
        gc.collect()
        assert rng.device_salt_ptr() == 0
    finally:
        rng.set_device_salt(None)
    assert rng.device_salt_ptr() == 0
