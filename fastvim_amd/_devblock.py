"""The writer of a small parameter block in device memory that captured launches read when they RUN (the mix-parameter
block of ``fastvim_amd.mixup.Mixup``, the channel indices of ``fastvim_amd.hcs.ChannelSampler``): the host rewrites the
block between two replays, the way ``FlatAdamW.set_lr`` feeds the optimizer graph its learning rate."""
import torch


class BlockWriter:
    """``write(block, words)``: an asynchronous copy of ``words`` (bytes, or a sequence of int32) from pinned memory into
    the int32 device tensor ``block`` on the current stream -- ordered before the next launch / replay, and the host does
    not wait for the step in flight.  A staging buffer is rewritten only once its own last copy is done (``slots`` take
    turns, so that is the copy of ``slots`` calls ago)."""

    def __init__(self, n_int32, slots=4):
        self.n = int(n_int32)
        self._host = [[torch.zeros(self.n, dtype=torch.int32).pin_memory(), None] for _ in range(slots)]     # [tensor, event of its last copy]
        self._turn = 0

    def write(self, block, words):
        if isinstance(words, (bytes, bytearray)):
            src = torch.frombuffer(bytearray(words), dtype=torch.int32)
        else:
            src = torch.tensor(list(words), dtype=torch.int32)
        if src.numel() > self.n or block.numel() < src.numel():
            raise ValueError(f"BlockWriter: {src.numel()} words do not fit the block ({block.numel()}) / the staging buffer ({self.n})")
        slot = self._host[self._turn]
        self._turn = (self._turn + 1) % len(self._host)
        if slot[1] is not None:
            slot[1].synchronize()
        slot[0][:src.numel()].copy_(src)
        block[:src.numel()].copy_(slot[0][:src.numel()], non_blocking=True)
        slot[1] = torch.cuda.Event()
        slot[1].record(torch.cuda.current_stream(block.device))
