"""The device Keccak round (theta and chi on 3-input bitwise ops) against
the C oracle's keccak256.

Every device kernel shares one keccak_f, so it is checked where a message
can be handed to it directly: keccak_batch_device (k_keccak_batch, one
block: its contract rejects 136 bytes and up, pinned in test_gpu_parity)
and keccak_long_device (k_keccak_long, any length), which carries the
multi-block lengths.

- message lengths 0, 1, 135, 136, 137, 271, 272, 273: the pad byte alone,
  the pad's 0x01 and 0x80 in one byte (135, 271), a pad-only last block
  (136, 272) and one byte into the next block (137, 273);
- all-zero and all-0xFF messages at each length;
- the 1,088 single-bit messages of one 136-byte block: each bit of the rate
  enters one state lane once, so a wrong truth table or a swapped operand of
  a 3-input op shows in a specific lane. The same bits (1,080 of them) also
  go through the one-block kernel as 135-byte messages.
"""
import numpy as np
import pytest
import torch

from oracle import bind

pytestmark = pytest.mark.gpu

LENS = [0, 1, 135, 136, 137, 271, 272, 273]
ONE_BLOCK_MAX = 135


@pytest.fixture(scope="module")
def eng():
    from reth_amd.engine import StateRootEngine
    e = StateRootEngine(0)
    yield e
    e.close()


def _want(msgs, msg_len):
    if msg_len == 0:
        return np.tile(np.frombuffer(bind.keccak256(b""), np.uint8),
                       (len(msgs), 1))
    return bind.keccak256_batch(np.ascontiguousarray(msgs[:, :msg_len]))


def _device(fn, msgs, msg_len):
    """Hash rows [:n] of a padded buffer; the rows past n stay untouched."""
    n = len(msgs)
    pad = np.full((256, msgs.shape[1]), 0x3C, np.uint8)
    t = torch.from_numpy(np.concatenate([msgs, pad])).cuda()
    out = torch.full((n + 256, 32), 0xA5, dtype=torch.uint8, device="cuda")
    fn(t[:n], msg_len, out[:n])
    got = out.cpu().numpy()
    assert (got[n:] == 0xA5).all(), f"wrote past n at len {msg_len}"
    return got[:n]


def _kernels(eng, msg_len):
    k = [("long", eng.keccak_long_device)]
    if msg_len <= ONE_BLOCK_MAX:
        k.append(("batch", eng.keccak_batch_device))
    return k


def _fixed_messages(msg_len):
    """all-zero, all-0xFF and two random rows, in a row of stride >= 8."""
    rng = np.random.default_rng(1000 + msg_len)
    stride = max(msg_len, 8)
    m = np.zeros((4, stride), np.uint8)
    m[1] = 0xFF
    m[2:] = rng.integers(0, 256, (2, stride), dtype=np.uint8)
    return m


@pytest.mark.parametrize("msg_len", LENS)
def test_lengths_zero_and_ff(eng, msg_len):
    msgs = _fixed_messages(msg_len)
    want = _want(msgs, msg_len)
    if msg_len:  # the reference itself: the oracle's single-message entry
        assert bytes(want[1]) == bind.keccak256(b"\xff" * msg_len)
    for name, fn in _kernels(eng, msg_len):
        got = _device(fn, msgs, msg_len)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert not len(bad), f"{name}, len {msg_len}, row {bad[0]} " \
            "(0 zero, 1 0xFF, 2-3 random)"


def _single_bit(nbytes):
    m = np.zeros((8 * nbytes, nbytes), np.uint8)
    bits = np.arange(8 * nbytes)
    m[bits, bits // 8] = 1 << (bits % 8)
    return m


def _report(got, want, name):
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert not len(bad), \
        f"{name}: {len(bad)} single-bit messages differ; first is bit " \
        f"{bad[0] % 64} of lane {bad[0] // 64}"


def test_single_bit_messages_of_one_block(eng):
    msgs = _single_bit(136)
    assert msgs.shape == (1088, 136)
    assert (np.unpackbits(msgs, axis=1).sum(axis=1) == 1).all()
    _report(_device(eng.keccak_long_device, msgs, 136), _want(msgs, 136),
            "long")


def test_single_bit_messages_one_block_kernel(eng):
    msgs = _single_bit(135)
    want = _want(msgs, 135)
    for name, fn in _kernels(eng, 135):
        _report(_device(fn, msgs, 135), want, name)
