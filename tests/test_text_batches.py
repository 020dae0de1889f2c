"""epilogos_amd/textBatches.py: the offset and growth arithmetic of the staging slots (no GPU), and on the GPU what the two readers
rely on when something goes wrong in the middle: a consumer that raises gets every inflated buffer back before the exception
leaves the `with` block, and a slot whose batch was never released is not staged again."""
import numpy as np
import pytest

from epilogos_amd import _io, textBatches as tb


def test_texts_start_16_byte_aligned():
    assert [tb.align(n, 16) for n in (0, 1, 15, 16, 17, 4096)] == [0, 16, 16, 16, 32, 4096]
    offs = tb.offsets_of([0, 1, 16, 17, 5])
    assert offs.dtype == np.int64 and offs.tolist() == [0, 0, 16, 32, 64, 80]
    assert tb.offsets_of([]).tolist() == [0]
    assert tb.offsets_of([3, 3], a=4).tolist() == [0, 4, 8]


def test_a_slot_grows_by_an_eighth_to_a_page_and_only_when_it_must():
    assert tb.slot_capacity(0) == 0 and tb.slot_capacity(1) == 4096 and tb.slot_capacity(4096) == 8192      # 4096 + 512 -> two pages
    assert tb.slot_capacity(7) == 4096 and tb.slot_capacity(3640) == 4096 and tb.slot_capacity(3641) == 4096 and tb.slot_capacity(3642) == 8192
    for total in (18064, 1 << 20, 192 * 1000 * 1000 + 5):
        cap = tb.slot_capacity(total)
        assert cap % 4096 == 0 and 0 <= cap - (total + total // 8) < 4096
        # a smaller request: no new buffer
        assert tb.slot_capacity(total - 1, cap) == cap and tb.slot_capacity(cap, cap) == cap and tb.slot_capacity(0, cap) == cap
        grown = tb.slot_capacity(cap + 1, cap)
        assert grown == tb.slot_capacity(cap + 1) and grown > cap


def test_pointers_are_the_rows_and_the_tails_of_a_tensor():
    import torch
    rows = torch.zeros((5, 3, 3), dtype=torch.int64)
    assert tb.pointers(rows) == [rows[i].data_ptr() for i in range(5)]
    lines = torch.zeros(40, dtype=torch.int32)
    assert tb.pointers(lines, np.array([0, 16, 32])) == [lines[s:].data_ptr() for s in (0, 16, 32)]
    assert tb.pointers(torch.zeros(0, dtype=torch.uint8), [0]) == [0]                 # no text at all: NULL, and the entry points say so


class _Counted(_io.Text):
    opened, closed = [], []

    def __init__(self, path, threads=0):
        super().__init__(path, threads)
        self.opened.append(str(path))

    def close(self):
        if not getattr(self, "counted", False):
            self.counted = True
            self.closed.append(1)
        super().close()


@pytest.fixture
def counted(tmp_path, monkeypatch):
    _Counted.opened, _Counted.closed = [], []
    monkeypatch.setattr(_io, "Text", _Counted)
    files = []
    for k in range(5):
        files.append(tmp_path / ("t%d.txt" % k))
        files[-1].write_bytes(b"text %d\n" % k * (k + 1))
    return files


@pytest.mark.gpu
def test_a_consumer_that_raises_gets_every_inflated_buffer_back(counted):
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    with pytest.raises(KeyError):
        with tb.TextBatches(counted, 2, 2, dev, lambda k, data: (k, len(data))) as batches:
            for b in batches:
                assert (b.k0, b.nb, b.sizes, b.facts) == (0, 2, [7, 14], [(0, 7), (1, 14)]) and b.offsets.tolist() == [0, 16, 32]
                for j in range(b.nb):
                    got = b.text[b.offsets[j]:b.offsets[j] + b.sizes[j]].cpu().numpy().tobytes()
                    assert got == counted[j].read_bytes()
                raise KeyError("the consumer")
    # the batch handed out and the one that was inflating behind it; the fifth file was never opened
    assert sorted(_Counted.opened) == [str(f) for f in counted[:4]] and len(_Counted.closed) == 4


@pytest.mark.gpu
def test_a_slot_that_was_never_released_is_not_staged_again(counted):
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    seen = []
    with tb.TextBatches(counted, 1, 2, dev, lambda k, data: None) as batches:
        with pytest.raises(RuntimeError):
            for b in batches:
                seen.append(b.k0)                                # no b.release()
    assert seen == [0, 1] and len(_Counted.closed) == len(_Counted.opened)
    seen = []
    with tb.TextBatches(counted, 1, 2, dev, lambda k, data: None) as batches:
        for b in batches:
            seen.append(b.k0)
            b.release()
    assert seen == [0, 1, 2, 3, 4] and len(_Counted.closed) == len(_Counted.opened) and batches.inflate_s > 0
