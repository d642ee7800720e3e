"""Guarded device buffers for the GPU tests of entry points that write into caller-owned memory (the
scheme of tests/test_gpu_composite_edges.py): the body lies between two guards of 1024 words, all
preset to a NaN bit pattern no kernel produces; after the call no guard word and no body word the
contract does not name may have changed, and every word it names must have."""
import torch

SENTINEL = 0x7FC0BEEF
GUARD = 1024


class Guarded:
    """n elements of dtype float32 / int32 (one word each) or int64 (two words each) between guards.
    `named` (bool [n], default all) marks the elements the contract writes."""

    def __init__(self, n, dtype=torch.float32, named=None, device="cuda"):
        self.words = 2 if dtype == torch.int64 else 1
        self.n = n
        self.flat = torch.full((2 * GUARD + n * self.words,), SENTINEL, dtype=torch.int32, device=device)
        self.body = self.flat[GUARD:GUARD + n * self.words].view(dtype)
        self.named = torch.ones(n, dtype=torch.bool) if named is None else named

    def ptr(self):
        return self.body.data_ptr()

    def check(self, what, written=True):
        bits = self.flat.cpu()
        keep = torch.ones(bits.numel(), dtype=torch.bool)
        if written:
            keep[GUARD:GUARD + self.n * self.words] = ~self.named.repeat_interleave(self.words)
        stray = int((bits[keep] != SENTINEL).sum())
        assert stray == 0, f"{what}: {stray} words stored outside the elements the contract names"
        if written and self.words == 1:
            missing = int((bits[~keep] == SENTINEL).sum())
            assert missing == 0, f"{what}: {missing} named elements never stored"
        elif written:
            # an int64 element is stored when either of its words changed (small indices leave the
            # high word 0, never the pattern)
            pairs = bits[~keep].view(-1, 2)
            missing = int(((pairs[:, 0] == SENTINEL) & (pairs[:, 1] == SENTINEL)).sum())
            assert missing == 0, f"{what}: {missing} named elements never stored"
