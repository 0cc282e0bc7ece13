"""The workspace policy the tests install (pafuse_amd._lib.workspace_policy): every byte arena the library hands to its C ABI
gets a guard band on either side and a chosen content.

    arenas = GuardedArenas("ones")
    with _lib.workspace_policy(arenas):
        out = model(...)
    arenas.check()          # no guard byte changed: nothing was written outside the bytes the *_bytes() call asked for
    arenas.names()          # the call sites that asked, in order

An arena is ONE uint8 tensor of GUARD + nbytes + GUARD bytes (the float64 arenas are a view of it): the guards hold the sentinel
0xA5, the interior holds `fill` - "zeros", "ones" (every byte 0xFF: a NaN as fp32, as an fp16 / bf16 pair and as fp64, -1 as
any integer) or "random" (bytes of a seeded generator: inf, NaN, denormals and huge integers all occur).  The view starts on a
256-byte boundary (the tensor is cut from a block 255 bytes longer; GUARD = 4096 keeps that alignment; the C ABI asks for 8).
Filling happens at allocation - in the graph path before the capture begins - so a fill is never recorded into a graph.
A plain module, not a conftest: nothing here runs unless a test installs it."""
import torch

GUARD = 4096
SENTINEL = 0xA5
FILLS = ("zeros", "ones", "random")


class GuardedArenas:
    def __init__(self, fill, seed=20240605, reuse=False):
        assert fill in FILLS, fill
        self.fill = fill
        self.seed = seed
        self.reuse = reuse    # True: a second request of the same (what, nbytes, dtype, device) gets the FIRST one's arena back as the
        #                       first call left it - a long-running process whose allocator hands a freed block to the same call site
        self.arenas = []      # (what, whole uint8 tensor, nbytes)
        self.requests = []    # what, per request
        self._views = {}

    def __call__(self, nbytes, device, what, dtype):
        self.requests.append(what)
        key = (what, nbytes, dtype, str(device))
        if self.reuse and key in self._views:
            return self._views[key]
        view = self._views[key] = self._new(nbytes, device, what, dtype)
        return view

    def _new(self, nbytes, device, what, dtype):
        raw = torch.empty(GUARD + nbytes + GUARD + 255, dtype=torch.uint8, device=device)
        skip = -raw.data_ptr() % 256        # (0 on the device; the host allocator aligns to 64 bytes only)
        whole = raw[skip:skip + GUARD + nbytes + GUARD]
        whole[:GUARD] = SENTINEL
        whole[GUARD + nbytes:] = SENTINEL
        inner = whole[GUARD:GUARD + nbytes]
        if self.fill == "zeros":
            inner.zero_()
        elif self.fill == "ones":
            inner.fill_(0xFF)
        else:       # a generator of the arena's device (an arena of the loop is 100 MB and more), seeded per arena
            g = torch.Generator(device=whole.device).manual_seed(self.seed + len(self.arenas))
            inner.copy_(torch.randint(0, 256, (nbytes,), dtype=torch.uint8, generator=g, device=whole.device))
        self.arenas.append((what, whole, nbytes))
        return inner if dtype == torch.uint8 else inner.view(dtype)

    def names(self):
        return list(self.requests)

    def check(self):
        """every guard byte of every arena still holds the sentinel, else an AssertionError naming the arena, the side and the
        first offset that differs (relative to the view: -1 is the byte just below it, nbytes the byte just behind it)"""
        if any(whole.is_cuda for _, whole, _ in self.arenas):
            torch.cuda.synchronize()
        for k, (what, whole, nbytes) in enumerate(self.arenas):
            for side, band, first in (("below", whole[:GUARD], -GUARD), ("above", whole[GUARD + nbytes:], nbytes)):
                bad = (band != SENTINEL).nonzero()
                if bad.numel():
                    at = int(bad[0])
                    raise AssertionError(f"arena #{k} '{what}' ({nbytes} bytes): guard {side} the view was written: first at offset "
                                         f"{first + at} of the view, {int(bad.numel())} guard bytes differ, byte there {int(band[at]):#04x}")
