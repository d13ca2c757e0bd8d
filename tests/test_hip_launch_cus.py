"""GPU test of the launch helpers' CU count (ctrlhair_amd/csrc/launch.h device_cus): a persistent launch with more tasks than compute
units has exactly one block per unit of the handle's device.

The count has no accessor, so it is read off the grid of a launch: with option sean.dbg bit 256 (DBG_STAMP, dbg_bits.h) wave 0 of every
block of the wave-specialised ACE conv writes cycle stamps of its tiles at block index x 64 x 3 words of the split-K scratch, which
ch_sean_debug_read copies out (tools/ws_timeline.py reads the same records).  The scratch also holds whatever split-K slabs earlier
layers left there, so the blocks are told from that by running twice: a stamp is a clock value and differs between the runs, the slabs
of two identical runs do not (every split-K reduction of the library adds its slabs in a fixed order; the test would fail, not pass, if
one did not).

256, the value the helper falls back to when the query fails, is also the CU count of an MI355X: on that device the test cannot tell a
failed query from a good one.  It does tell a count taken from anything else."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_persistent_grid_is_the_devices_cu_count(hip_lib):
    from ctrlhair_amd import procedural as P
    from ctrlhair_amd.sean.generator import SeanGenerator
    # ACE 16 (the default sean.dbg_sel) runs at S x S: dense (sean.sparse 0, every block has tiles from its first step on) it has
    # ceil(C / 32) x S / 32 x S / 16 x B >= 512 tiles of 32 x 16 pixels, two rounds of the 256 units of an MI355X
    ngf, S, B, NBLK = 16, 256, 4, 512
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert 0 < cus < NBLK, cus
    gen = SeanGenerator(0, f16x3=1, options={'sean.sparse': 0}).load_state_dict(P.sean_state_dict(0, ngf), max_batch=B, max_size=S)
    dev = gen.device
    args = [torch.from_numpy(a).to(dev) for a in (P.blocky_labels(B, S, grid=8), P.style_codes(B), P.noise_planes(B, S, ngf))]
    gen.handle.set_option('sean.dbg', 64 | 256)          # the wave-specialised kernel for every eligible ACE, stamps of ACE 16
    snaps = []
    for _ in range(2):
        gen.generate(*args)
        torch.cuda.synchronize()
        buf = np.zeros(NBLK * 64 * 3, np.int64)
        gen.handle._check(gen.handle.lib.ch_sean_debug_read(gen.handle._h, buf.ctypes.data_as(C.c_void_p), buf.nbytes), 'ch_sean_debug_read')
        snaps.append(buf.reshape(NBLK, 64, 3)[:, 0, :].copy())        # first tile of every block: start, end of k-loop, end of epilogue
    a, b = snaps
    ran = (a[:, 0] != b[:, 0]) & (a[:, 0] < a[:, 1]) & (a[:, 1] < a[:, 2]) & (b[:, 0] < b[:, 1]) & (b[:, 1] < b[:, 2])
    print(f'stamped blocks among the first {NBLK}: {int(ran.sum())}, multi_processor_count {cus}')
    # only blocks 0 .. cus are judged, so what other layers leave further up in the scratch cannot count as a block
    assert ran[:cus].all(), f'blocks {np.flatnonzero(~ran[:cus])[:8]} below the CU count left no stamps: the grid is smaller'
    assert (a[cus] == b[cus]).all(), 'block number multi_processor_count ran: the grid is larger'
