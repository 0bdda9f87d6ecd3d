"""Prefix KV cache: the talker K/V rows of a voice's instruct turn, kept on the device and reused by later requests.

The instruct rows come first in the talker prompt and are text only (``prompt.py``, ``model.py::_build_talker_inputs_local``);
attention is causal, so in every layer their K/V rows depend on the instruct ids alone.  The prompt builder notes them on the
embeddings (``tie.fq3_prefix = (rows, ids)``) and ``generate._prefill_first_token`` hands the note to :meth:`PrefixCache.prefill`:

* **miss**: the engine prefills the ``P`` prefix rows (``fq3_prefill``), the cache saves them into an entry
  (``entry.kv_copy(engine, P)``), the engine continues with the rest (``fq3_prefill_continue``);
* **hit**: the engine receives the entry's rows (``engine.kv_copy(entry, P)``) and continues with the rest.

Both run the same continuation on the same prefix bits -- the copy is exact -- so a request gives the same codes whether or not its
voice was cached.  An entry is a pooled context that never prefills (so it never allocates a prefill workspace): it shares the
engine's weights and holds ``ceil(P / 64)`` blocks of the cache's own KV pool of ``capacity_rows / 64`` blocks.

A lock-step batch scheduler hands a whole admitted group to :meth:`PrefixCache.prefill_pack`: the members without a usable prefix go
through the plain packed prefill, each distinct missing prefix is prefilled once, and every member behind a prefix continues in ONE
packed continuation (``fq3_prefill_continue_batch``).

**One stream.**  All cache work is enqueued on the engine's current stream.  Eviction hands an entry's blocks back to the pool on
the host at once, and the next save overwrites them: that is safe only because every copy out of and into those blocks is ordered
on that one stream.  Do not share a cache between engines that run on different streams; the object is not re-entrant either (the
server uses it under its one-request-at-a-time lock).  A cache handed to a ``BatchDecoder`` serves that scheduler alone: all its work
is queued on the stream the scheduler prefills on.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, Optional

from . import _lib as L
from .engine import KV_BLOCK

# The smallest probed prefix at which a hit beats the plain prefill on both model sizes (tools/prefix_cache_probe.py ->
# profiles/prefix_cache.json): 64 rows, one KV block -- a hit won at every probed prefix.
DEFAULT_MIN_ROWS = 64
# The same for a batch scheduler's packed admission (profiles/prefix_cache_batch.json).
DEFAULT_BATCH_MIN_ROWS = 64


def _blocks(rows: int) -> int:
    return (int(rows) + KV_BLOCK - 1) // KV_BLOCK


class PrefixCache:
    def __init__(self, engine, capacity_rows: int, min_rows: Optional[int] = None):
        """``engine``: the generating engine (its shape, dtype and weights are the entries').  ``capacity_rows``: K/V rows the cache
        may hold, in whole 64-row blocks.  ``min_rows``: shorter prefixes are not worth a copy and a second pass (bypass)."""
        self.capacity_blocks = int(capacity_rows) // KV_BLOCK
        if self.capacity_blocks < 1:
            raise ValueError("PrefixCache: capacity_rows must hold at least one 64-row KV block")
        self.min_rows = DEFAULT_MIN_ROWS if min_rows is None else int(min_rows)
        self.engine = engine
        self.pool = engine.kv_pool(self.capacity_blocks)
        self._entries: "OrderedDict[tuple, tuple]" = OrderedDict()      # key -> (entry context, P), least recently used first
        self._spare = []                                               # contexts of evicted entries (they own no block)
        self._n = dict(hits=0, misses=0, bypasses=0, evictions=0, rows_reused=0)

    # ------------------------------------------------------------------------------------------
    @staticmethod
    def _key(engine, ids) -> tuple:
        return (tuple(int(i) for i in ids), str(engine.dtype), id(getattr(engine, "_table", None)))

    def _usable(self, x, n_pad: int, note) -> int:
        """The prefix rows to go through the cache, or 0 (bypass)."""
        if not (isinstance(note, tuple) and len(note) == 2) or n_pad != 0:
            return 0
        P, ids = int(note[0]), note[1]
        if P <= 0 or P != len(ids) or P < self.min_rows or _blocks(P) > self.capacity_blocks or P >= int(x.shape[0]):
            return 0
        return P

    def _evict_lru(self) -> bool:
        if not self._entries:
            return False
        _key, (ctx, _P) = self._entries.popitem(last=False)
        ctx.kv_release(0)              # host side, at once: see the module docstring (one stream)
        self._spare.append(ctx)
        self._n["evictions"] += 1
        return True

    def _save(self, engine, key, P: int) -> None:
        ctx = self._spare.pop() if self._spare else self.engine.spawn_pooled(self.pool)
        while True:
            try:
                ctx.kv_copy(engine, P)
                break
            except L.Fq3Error as e:
                if e.code != L.FQ3_ENOMEM or not self._evict_lru():
                    self._spare.append(ctx)
                    if e.code != L.FQ3_ENOMEM:
                        raise
                    return             # nothing left to evict (cannot happen: P fits the capacity); the request goes on uncached
        self._entries[key] = (ctx, P)

    # ------------------------------------------------------------------------------------------
    def prefill(self, engine, x, n_pad: int = 0, note=None):
        """The prefill of prompt rows ``x`` [L, H] on ``engine`` -> (logits, hidden), through the cache when ``note`` (the prompt
        builder's ``fq3_prefix``) names a usable prefix; the plain ``engine.prefill`` otherwise."""
        P = self._usable(x, n_pad, note)
        if P == 0:
            self._n["bypasses"] += 1
            return engine.prefill(x, n_pad=n_pad)
        key = self._key(engine, note[1])
        hit = self._entries.get(key)
        if hit is not None:
            self._entries.move_to_end(key)
            engine.kv_copy(hit[0], P)
            self._n["hits"] += 1
            self._n["rows_reused"] += P
        else:
            engine.prefill(x[:P], n_pad=0, want_logits=False)
            self._save(engine, key, P)
            self._n["misses"] += 1
        return engine.prefill_continue(x[P:], P)

    @staticmethod
    def _runs(idx, rows, cap):
        """``idx`` cut into runs whose ``rows`` sum to at most ``cap`` (a packed pass runs on one context's workspace)."""
        out, cur, tot = [], [], 0
        for i, r in zip(idx, rows):
            if cur and tot + r > cap:
                out.append(cur)
                cur, tot = [], 0
            cur.append(i)
            tot += r
        if cur:
            out.append(cur)
        return out

    def prefill_pack(self, engines, xs, pads, notes):
        """:meth:`prefill` for a group a batch scheduler admits together: ``xs[i]`` [L_i, H] into ``engines[i]`` (contexts of one
        weight table), ``pads[i]`` its left padding, ``notes[i]`` its ``fq3_prefix`` note or None.  Returns ``[(logits, hidden), ...]``
        in request order; everything is queued on the current stream and nothing is waited for.

        Members without a usable prefix go through one plain ``Fq3Engine.prefill_batch``.  Of the others, a hit receives the entry's
        rows; each DISTINCT missing key is prefilled once, into the first member that names it (several of them in one packed pass
        without logits), saved, and copied to the other members of that key -- those count as hits.  Then all of them continue in one
        ``Fq3Engine.prefill_continue_batch``.  The members' contexts may already own the blocks of their whole utterance: a copy
        into them takes none."""
        from .engine import Fq3Engine
        n = len(engines)
        res = [None] * n
        cap = int(getattr(engines[0], "max_seq_len", 1 << 30))
        Ps = [self._usable(x, int(p), nt) for x, p, nt in zip(xs, pads, notes)]
        rest = [i for i in range(n) if Ps[i] == 0]
        use = [i for i in range(n) if Ps[i] > 0]
        self._n["bypasses"] += len(rest)
        for run in self._runs(rest, [int(xs[i].shape[0]) for i in rest], cap):
            outs = Fq3Engine.prefill_batch([engines[i] for i in run], [xs[i] for i in run], [int(pads[i]) for i in run])
            for i, o in zip(run, outs):
                res[i] = o
        if not use:
            return res
        first = {}                        # missing key -> the member that prefills it
        followers = []                    # (member, key): named a key that missed earlier in this group
        for i in use:
            key = self._key(engines[i], notes[i][1])
            if key in first:
                followers.append((i, key))
                self._n["hits"] += 1
                self._n["rows_reused"] += Ps[i]
                continue
            hit = self._entries.get(key)
            if hit is not None:
                self._entries.move_to_end(key)
                engines[i].kv_copy(hit[0], Ps[i])
                self._n["hits"] += 1
                self._n["rows_reused"] += Ps[i]
            else:
                first[key] = i
                self._n["misses"] += 1
        miss = list(first.values())
        for run in self._runs(miss, [Ps[i] for i in miss], cap):
            if len(run) == 1:
                i = run[0]
                engines[i].prefill(xs[i][:Ps[i]], n_pad=0, want_logits=False)
            else:
                Fq3Engine.prefill_batch([engines[i] for i in run], [xs[i][:Ps[i]] for i in run], [0] * len(run), want_logits=False)
        for key, i in first.items():
            self._save(engines[i], key, Ps[i])
        for j, key in followers:          # from the member that holds the rows: the entry may already have been evicted again
            engines[j].kv_copy(engines[first[key]], Ps[j])
        for run in self._runs(use, [int(xs[i].shape[0]) - Ps[i] for i in use], cap):
            outs = Fq3Engine.prefill_continue_batch([engines[i] for i in run], [xs[i][Ps[i]:] for i in run], [Ps[i] for i in run])
            for i, o in zip(run, outs):
                res[i] = o
        return res

    def stats(self) -> Dict[str, int]:
        held = sum(_blocks(P) for _ctx, P in self._entries.values())
        return dict(self._n, entries=len(self._entries), blocks_held=held, blocks_capacity=self.capacity_blocks)

    def clear(self) -> None:
        """Drop every entry (their blocks go back to the cache's pool); the counters stay."""
        for ctx, _P in self._entries.values():
            ctx.kv_release(0)
            self._spare.append(ctx)
        self._entries.clear()

    def close(self) -> None:
        self.clear()
        for ctx in self._spare:
            ctx.close()
        self._spare = []
        if self.pool is not None:
            self.pool.close()
            self.pool = None
