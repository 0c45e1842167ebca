"""The opt-in device-side embedding exchange (``ShardedEmbedding(exchange="device")``,
``parallel/sparse_exchange.py``) as far as a machine without a GPU sees it: the option
resolves, a CPU table keeps the host path, batch preparation plans on the host only for
host-mode tables, and the kernels' entry points refuse bad arguments before any launch."""
import ctypes

import pytest
import torch


class _Loop:
    """A communicator of "two ranks" of which this one owns every row: whatever rank 0
    sends itself comes straight back, rank 1 sends and receives nothing."""

    def all_to_all_single(self, out, inp, out_splits, in_splits):
        out.reshape(-1)[:inp.numel()].copy_(inp.reshape(-1))


def _two_rank_table(**kw):
    from kubeflow_controller_amd.parallel.embedding import ShardedEmbedding
    emb = ShardedEmbedding(100, 8, optimizer="sgd", lr=0.5, device="cpu", **kw)
    emb.world, emb.comm = 2, _Loop()   # owners stays 1: rank 0 holds the whole table
    return emb


def test_exchange_option_resolves(monkeypatch):
    from kubeflow_controller_amd.parallel.embedding import ShardedEmbedding
    monkeypatch.delenv("KFA_EMB_EXCHANGE", raising=False)
    assert ShardedEmbedding(10, 8).exchange == "host"
    assert ShardedEmbedding(10, 8, exchange="device").exchange == "device"
    monkeypatch.setenv("KFA_EMB_EXCHANGE", "device")
    assert ShardedEmbedding(10, 8).exchange == "device"
    assert ShardedEmbedding(10, 8, exchange="host").exchange == "host"   # the argument wins
    monkeypatch.setenv("KFA_EMB_EXCHANGE", "gpu")
    with pytest.raises(ValueError, match="exchange"):
        ShardedEmbedding(10, 8)
    with pytest.raises(ValueError, match="exchange"):
        ShardedEmbedding(10, 8, exchange="nccl")


@pytest.mark.parametrize("exchange", ["device", "host"])
def test_cpu_table_keeps_the_host_path(exchange):
    emb = _two_rank_table(exchange=exchange)
    w0 = emb.weight.detach().clone()
    ids = torch.tensor([3, 7, 3, 3, 99, 7])
    out = emb(ids)
    assert emb.exchange_bytes["path"] == "host"
    assert emb.exchange_bytes["lookups"] == 6 and emb.exchange_bytes["sent_ids"] == 3
    assert torch.equal(out, w0[ids])
    out.backward(torch.ones(6, 8))
    want = w0.clone()
    want[3] -= 0.5 * 3   # lr * occurrences
    want[7] -= 0.5 * 2
    want[99] -= 0.5 * 1
    torch.testing.assert_close(emb.weight.detach(), want)


def test_config_reaches_the_table_and_batches_carry_no_host_plan():
    from kubeflow_controller_amd.models.wide_deep import WideDeep, WideDeepConfig, prepare_batch, synthetic_batch
    made = {}
    for mode in (None, "device"):
        cfg = WideDeepConfig.tiny()
        cfg.exchange = mode
        m = WideDeep(cfg, device="cpu")
        assert m.tables.exchange == (mode or "host")
        m.tables.world = 2
        m.tables.plan = lambda gids: ([int(gids.numel()), 0], [int(gids.numel()), 0], None, None)
        made[mode] = prepare_batch(m, *synthetic_batch(cfg, 4, torch.Generator().manual_seed(0)), "cpu")[1]
    assert hasattr(made[None], "_kfa_plan") and made[None]._kfa_plan[0] == [32, 0]
    assert not hasattr(made["device"], "_kfa_plan")


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """No device is touched: every check comes before the first HIP call."""
    from kubeflow_controller_amd.ops import _lib
    from kubeflow_controller_amd.parallel import sparse_exchange as X  # noqa: F401 - registers the signatures
    lib = _lib.lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    big = 2 ** 31
    assert lib.kfa_xchg_ws_bytes(big) == 0 and lib.kfa_xchg_ws_bytes(4097) > 4 * 4097 * 4
    assert lib.kfa_xchg_part_floats(65, 72) == 2 * 2 * 72
    plan = lambda n, world, owners, R, rows, ws: lib.kfa_xchg_plan(p, n, world, owners, R, rows, p, ws, p, p, p, p,  # noqa: E731
                                                                     None)
    assert plan(big, 2, 2, 500, 1000, 1 << 40) != 0            # n > 2^31 - 1
    assert plan(64, 2, 2, 2 ** 31 + 1, 1000, 1 << 40) != 0     # owners * rows_per_owner > 2^32
    assert plan(64, 2, 3, 500, 1000, 1 << 40) != 0             # more owners than ranks
    assert plan(64, 2, 2, 500, 1001, 1 << 40) != 0             # more rows than the owners hold
    assert plan(64, 2, 2, 500, 1000, 16) != 0                  # short workspace
    assert lib.kfa_xchg_expand(p, 4, p, 64, 12, p, None) != 0  # D % 8
    assert lib.kfa_xchg_expand(p, 4, p, big, 8, p, None) != 0
    presum = lambda n, D, U, ws, pf: lib.kfa_xchg_presum(p, n, D, U, p, ws, p, p, p, pf, p, None)  # noqa: E731
    assert presum(64, 12, 4, 1 << 40, 1 << 40) != 0            # D % 8
    assert presum(64, 256, 4, 1 << 40, 1 << 40) != 0           # D > 248
    assert presum(big, 8, 4, 1 << 40, 1 << 40) != 0
    assert presum(64, 8, 65, 1 << 40, 1 << 40) != 0            # more distinct rows than entries
    assert presum(64, 8, 4, 16, 1 << 40) != 0                  # short workspace
    assert presum(64, 8, 4, 1 << 40, 8) != 0                   # short partial buffer
