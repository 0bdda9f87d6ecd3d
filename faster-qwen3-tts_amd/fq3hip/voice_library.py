"""Is this voice already enrolled, or on a list of voices that must not be cloned?  The nearest library voices of many clips.

Host side of ``fq3_voices_*``: a ``VoiceLibrary`` keeps up to ``capacity`` speaker embeddings on the device,
unit length, in the layout the scan kernel streams; ``search`` ranks the library against up to 32 queries per call in three launches
-- the library crosses HBM once, the scores are never written to memory -- and all queries' results reach the host behind one pinned
copy.  The order is (cosine descending, index ascending) and does not depend on the library's size or the other queries.

No threshold is chosen here: what cosine means "the same voice" depends on the checkpoint's speaker encoder (section 4.25).
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L

QUERY_MAX, K_MAX = 32, 16                                                   # rows and k of one fq3_voices_search call


class VoiceLibrary:
    """Named speaker embeddings on the device.  ``add`` / ``drop`` / ``search`` / ``save`` / ``load`` / ``len``."""

    def __init__(self, dim: int, capacity: int, device="cuda"):
        self.dim, self.capacity, self.device = int(dim), int(capacity), torch.device(device)
        self.names: List[Optional[str]] = []                                # by library index; None: dropped
        self._index = {}                                                    # name -> library index
        self._raw: List[np.ndarray] = []                                    # the embeddings as they were given (what save() writes)
        self.h = None
        self._create()

    # ---- the library calls (the tests' stand-ins replace these four) ----------------------------------------------------------------
    def _create(self) -> None:
        self.lib = L.load()
        h = L.vp()
        with torch.cuda.device(self.device):
            L.check(self.lib.fq3_voices_create(self.dim, self.capacity, C.byref(h)))
        self.h = h

    def _add_call(self, embeds: torch.Tensor) -> int:
        with torch.cuda.device(self.device):
            first = int(self.lib.fq3_voices_add(self.h, embeds.data_ptr(), embeds.shape[0], torch.cuda.current_stream(self.device).cuda_stream))
        if first < 0:
            L.check(first)
        return first

    def _drop_call(self, index: int) -> None:
        with torch.cuda.device(self.device):
            L.check(self.lib.fq3_voices_drop(self.h, index, torch.cuda.current_stream(self.device).cuda_stream))

    def _search_call(self, q: torch.Tensor, k: int, idx: torch.Tensor, cos: torch.Tensor) -> None:
        with torch.cuda.device(self.device):
            L.check(self.lib.fq3_voices_search(self.h, q.data_ptr(), q.shape[0], k, idx.data_ptr(), cos.data_ptr(),
                                               torch.cuda.current_stream(self.device).cuda_stream))

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.fq3_voices_destroy(self.h)
                self.h = None
        except Exception:
            pass

    # ---- the public interface -----------------------------------------------------------------------------------------------------
    def __len__(self) -> int:
        return len(self._index)

    def _rows(self, embeds) -> torch.Tensor:
        e = torch.as_tensor(embeds).to(dtype=torch.float32)
        e = e.reshape(-1, e.shape[-1]) if e.dim() != 2 else e
        if e.shape[-1] != self.dim:
            raise ValueError(f"embeddings of {e.shape[-1]} values; this library holds {self.dim}")
        return e

    def add(self, embeds, names: Sequence[str]) -> int:
        """Append ``embeds`` ``[n, dim]`` (tensor or array, any device) under ``names`` (n new, distinct strings) -> the first index."""
        e, names = self._rows(embeds), [str(n) for n in names]
        if len(names) != e.shape[0] or len(set(names)) != len(names) or any(n in self._index for n in names):
            raise ValueError("add: one new, distinct name per embedding")
        if not names:
            return len(self.names)
        first = self._add_call(e.to(self.device).contiguous())
        assert first == len(self.names)
        host = e.detach().cpu().numpy()
        for i, n in enumerate(names):
            self._index[n] = first + i
            self.names.append(n)
            self._raw.append(host[i])
        return first

    def drop(self, name: str) -> None:
        """``name`` is never returned again; the other voices keep their indices."""
        index = self._index.pop(name)                                       # KeyError: no such voice
        self._drop_call(index)
        self.names[index] = None

    def search(self, embeds, k: int = 1) -> List[List[Tuple[str, float]]]:
        """Per query embedding the ``k`` nearest live voices, best first: ``[(name, cosine), ...]`` (fewer than k when the library
        holds fewer).  Queries go in slices of 32, nothing is synchronised between slices, one pinned copy brings all results."""
        if not 1 <= int(k) <= K_MAX:
            raise ValueError(f"k = {k} outside [1, {K_MAX}]")
        q = self._rows(embeds).to(self.device).contiguous()
        n, k = q.shape[0], int(k)
        if n == 0:
            return []
        idx = torch.empty(n, k, dtype=torch.int32, device=self.device)
        cos = torch.empty(n, k, dtype=torch.float32, device=self.device)
        for lo in range(0, n, QUERY_MAX):
            self._search_call(q[lo: lo + QUERY_MAX], k, idx[lo: lo + QUERY_MAX], cos[lo: lo + QUERY_MAX])
        both = torch.cat([idx, cos.view(torch.int32)], dim=1)                # one copy for both halves
        host = both
        if both.is_cuda:
            host = torch.empty(both.shape, dtype=torch.int32, pin_memory=True)
            host.copy_(both, non_blocking=True)
            torch.cuda.current_stream(self.device).synchronize()
        hi, hc = host[:, :k].numpy(), host[:, k:].contiguous().view(torch.float32).numpy()
        return [[(self.names[int(i)], float(c)) for i, c in zip(hi[r], hc[r]) if i >= 0] for r in range(n)]

    def save(self, path) -> None:
        """The live voices as an ``.npz``: ``embeds`` float32 [n, dim] as they were given, ``names``, ``dim``."""
        keep = [i for i, n in enumerate(self.names) if n is not None]
        embeds = np.stack([self._raw[i] for i in keep]) if keep else np.zeros((0, self.dim), np.float32)
        with open(path, "wb") as f:
            np.savez(f, embeds=embeds.astype(np.float32), names=np.array([self.names[i] for i in keep], dtype=np.str_), dim=np.int64(self.dim))

    @classmethod
    def load(cls, path, device="cuda", capacity: Optional[int] = None) -> "VoiceLibrary":
        """A library from ``save``'s file; the device layout is rebuilt by ``add``.  ``capacity``: default the file's rows, at least 1024."""
        with np.load(path) as z:
            embeds, names, dim = z["embeds"], [str(n) for n in z["names"]], int(z["dim"])
        out = cls(dim, capacity if capacity is not None else max(len(names), 1024), device)
        if names:
            out.add(embeds, names)
        return out
