"""Block-table paged KV cache with per-sequence lengths (bf16 and fp8).

The serving-side cache for `tree_attn_decode_paged`: instead of one dense
(b, hk, n, d) tensor whose `n` is shared by the whole batch, K/V live in a
pool of fixed-size pages and every sequence owns a row of a block table:

    k_pages, v_pages   (num_pages, hk, page_size, D)   bf16, or uint8 e4m3
    k_scales, v_scales (num_pages, hk, page_size)      uint8 e8m0(+127), fp8 only
    block_table        int32 (max_seqs, max_pages_per_seq)
    seq_lens           int32 (max_seqs,)   tokens held per sequence, 0 is legal

Key j of sequence b lives at page block_table[b, j // page_size], row
j % page_size.  Table entries at or beyond ceil(seq_len / page_size) hold -1
and are never dereferenced.  D is the kernel head dim: 64 or 128; a smaller
`dim_head` is stored zero-padded to the next of those (exact: padded q/k dims
add 0 to the score, padded v dims are sliced off) while the softmax scale
stays `dim_head ** -0.5`.  The value dim equals the key dim on the paged path
(dv == d).  The fp8 pool is exactly `quantize_kv_cache`'s per-row format.

Page allocation is host-side: a free list plus a host mirror of the lengths
and the table, so appending and decoding never read anything back from the
device (no `.item()` on the step path).

Sliding-window serving: `release_prefix(keep_from)` hands back the pages of a
sequence that lie wholly below a position the caller will never attend again.
Positions stay ABSOLUTE: key j keeps table slot j // page_size for life, a
released slot holds -1, `append` continues at seq_len, and
`max_pages_per_seq` still bounds the absolute length (a ring-indexed table
that would reuse the released slots is out of scope).  `host_starts[s]` is the
number of released tokens; the attention entry points refuse, on the host and
before any launch, a call that would attend below it.
"""

from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import Tensor


def _kernel_dim(d: int) -> int:
    assert 0 < d <= 128, "paged cache: head dim <= 128"
    return 64 if d <= 64 else 128


class PagedKVCache:
    """Pool + block table + lengths for `max_seqs` sequences on one rank.

    append(k, v, lens) writes new tokens (HIP append kernel on GPU: a 16-byte
    row copy for bf16, fused per-row e8m0/e4m3 quantisation for fp8) and
    advances the lengths; free(seq) returns a sequence's pages;
    release_prefix(keep_from) returns the pages below a lookback window;
    gather(seq) rebuilds a dense (k, v) for debugging and tests.
    """

    def __init__(self, num_pages: int, page_size: int, kv_heads: int,
                 dim_head: int, max_seqs: int, max_pages_per_seq: int,
                 fp8: bool = False, device="cpu"):
        assert 16 <= page_size <= 256 and page_size & (page_size - 1) == 0, \
            "page_size must be a power of two in [16, 256]"
        self.num_pages, self.page_size = int(num_pages), int(page_size)
        self.kv_heads, self.dim_head = int(kv_heads), int(dim_head)
        self.kernel_dim = _kernel_dim(dim_head)
        self.max_seqs, self.max_pages_per_seq = int(max_seqs), int(max_pages_per_seq)
        self.fp8 = bool(fp8)
        self.device = torch.device(device)

        shape = (self.num_pages, self.kv_heads, self.page_size, self.kernel_dim)
        if self.fp8:
            self.k_pages = torch.zeros(shape, dtype=torch.uint8, device=self.device)
            self.v_pages = torch.zeros(shape, dtype=torch.uint8, device=self.device)
            self.k_scales = torch.zeros(shape[:3], dtype=torch.uint8, device=self.device)
            self.v_scales = torch.zeros(shape[:3], dtype=torch.uint8, device=self.device)
        else:
            self.k_pages = torch.zeros(shape, dtype=torch.bfloat16, device=self.device)
            self.v_pages = torch.zeros(shape, dtype=torch.bfloat16, device=self.device)
            self.k_scales = self.v_scales = None
        self.block_table = torch.full((self.max_seqs, self.max_pages_per_seq), -1,
                                      dtype=torch.int32, device=self.device)
        self.seq_lens = torch.zeros(self.max_seqs, dtype=torch.int32, device=self.device)

        # host-side allocator state: pages are handed out from the END of
        # the free list; _pages[s] mirrors the valid prefix of table row s
        # (-1 in the slots release_prefix has freed, _starts[s] // page_size
        # of them)
        self._free: list[int] = list(range(self.num_pages - 1, -1, -1))
        self._pages: list[list[int]] = [[] for _ in range(self.max_seqs)]
        self._lens: list[int] = [0] * self.max_seqs
        self._starts: list[int] = [0] * self.max_seqs

    # ---- host-side views ------------------------------------------------
    @property
    def host_lens(self) -> list[int]:
        return list(self._lens)

    @property
    def host_starts(self) -> list[int]:
        """Released tokens per sequence: keys below host_starts[s] are gone."""
        return list(self._starts)

    @property
    def max_seq_len(self) -> int:
        return max(self._lens) if self._lens else 0

    @property
    def free_pages(self) -> int:
        return len(self._free)

    def pages_of(self, seq: int) -> list[int]:
        """Page ids by table slot; a slot freed by release_prefix reads -1."""
        return list(self._pages[seq])

    def pages_held(self, seq: int | None = None) -> int:
        """Pages currently owned by `seq` (default: by all sequences)."""
        rows = self._pages if seq is None else [self._pages[seq]]
        return sum(pg >= 0 for row in rows for pg in row)

    # ---- construction helpers -------------------------------------------
    @classmethod
    def from_pages(cls, k_pages: Tensor, v_pages: Tensor, block_table: Tensor,
                   seq_lens: Tensor, k_scales: Tensor | None = None,
                   v_scales: Tensor | None = None,
                   dim_head: int | None = None) -> "PagedKVCache":
        """Adopt pools / table / lengths built elsewhere (no copy).  Reads
        the table and lengths back ONCE to build the host mirror; pages not
        referenced by a valid table entry form the free list."""
        num_pages, hk, page_size, kd = k_pages.shape
        fp8 = k_pages.dtype == torch.uint8
        assert (k_scales is not None) == fp8 and (v_scales is not None) == fp8
        self = cls.__new__(cls)
        self.num_pages, self.page_size = num_pages, page_size
        assert 16 <= page_size <= 256 and page_size & (page_size - 1) == 0
        self.kv_heads, self.kernel_dim = hk, kd
        self.dim_head = kd if dim_head is None else dim_head
        assert kd == _kernel_dim(self.dim_head)
        self.max_seqs, self.max_pages_per_seq = block_table.shape
        self.fp8, self.device = fp8, k_pages.device
        self.k_pages, self.v_pages = k_pages, v_pages
        self.k_scales, self.v_scales = k_scales, v_scales
        self.block_table, self.seq_lens = block_table, seq_lens
        self._lens = [int(x) for x in seq_lens.tolist()]
        self._starts = [0] * len(self._lens)
        table = block_table.tolist()
        self._pages = [table[s][:-(-n // page_size)]
                       for s, n in enumerate(self._lens)]
        used = {pg for row in self._pages for pg in row}
        assert all(0 <= pg < num_pages for pg in used), "invalid page id in a valid slot"
        assert len(used) == sum(len(r) for r in self._pages), "page referenced twice"
        self._free = [pg for pg in range(num_pages - 1, -1, -1) if pg not in used]
        return self

    @classmethod
    def from_dense(cls, k: Tensor, v: Tensor, seq_lens, page_size: int,
                   fp8: bool = False, shuffle_seed: int | None = None,
                   spare_pages: int = 0) -> "PagedKVCache":
        """Build a cache from dense (b, hk, n, d) k/v holding seq_lens[i]
        tokens of sequence i.  With `shuffle_seed` the page assignment is a
        seeded random permutation of the pool (otherwise ascending)."""
        b, hk, n, d = k.shape
        lens = [int(x) for x in (seq_lens.tolist() if isinstance(seq_lens, Tensor)
                                 else seq_lens)]
        assert len(lens) == b and all(0 <= x <= n for x in lens)
        per_seq = [-(-x // page_size) for x in lens]
        cache = cls(sum(per_seq) + spare_pages, page_size, hk, d, b,
                    max(max(per_seq), 1), fp8=fp8, device=k.device)
        if shuffle_seed is not None:
            gen = torch.Generator().manual_seed(shuffle_seed)
            cache._free = torch.randperm(cache.num_pages, generator=gen).tolist()
        t = max(lens)
        if t > 0:
            cache.append(k[:, :, :t], v[:, :, :t], lens)
        return cache

    # ---- mutation -------------------------------------------------------
    def append(self, k: Tensor, v: Tensor, lens=None) -> None:
        """Append tokens: k, v (max_seqs, hk, T, d); sequence i takes its
        first lens[i] tokens (default T for all; a host list keeps the step
        free of device reads).  Raises RuntimeError BEFORE writing anything
        if the pool or a table row would overflow."""
        b, hk, t, d = k.shape
        assert v.shape == k.shape, "paged path requires dv == d"
        assert b == self.max_seqs and hk == self.kv_heads and d == self.dim_head
        if lens is None:
            lens = [t] * b
        elif isinstance(lens, Tensor):
            lens = lens.tolist()
        lens = [int(x) for x in lens]
        assert len(lens) == b and all(0 <= x <= t for x in lens)

        # plan host-side first: nothing is touched if any check fails
        need = []
        for s in range(b):
            total = -(-(self._lens[s] + lens[s]) // self.page_size)
            if total > self.max_pages_per_seq:
                raise RuntimeError(
                    f"paged cache: sequence {s} needs {total} pages, table rows "
                    f"hold {self.max_pages_per_seq}")
            need.append(total - len(self._pages[s]))
        if sum(need) > len(self._free):
            raise RuntimeError(
                f"paged cache: pool exhausted ({sum(need)} pages needed, "
                f"{len(self._free)} free)")

        flat_idx, new_ids = [], []
        for s in range(b):
            for _ in range(need[s]):
                pg = self._free.pop()
                flat_idx.append(s * self.max_pages_per_seq + len(self._pages[s]))
                new_ids.append(pg)
                self._pages[s].append(pg)
        if new_ids:
            self.block_table.view(-1).index_copy_(
                0, torch.tensor(flat_idx, dtype=torch.long).to(self.device),
                torch.tensor(new_ids, dtype=torch.int32).to(self.device))

        if any(lens):
            append_lens = torch.tensor(lens, dtype=torch.int32).to(self.device)
            if self.device.type == "cuda":
                self._append_hip(k, v, append_lens)
            else:
                self._append_eager(k, v, lens)
            self.seq_lens += append_lens
            for s in range(b):
                self._lens[s] += lens[s]

    def _pad(self, x: Tensor) -> Tensor:
        d = x.shape[-1]
        return F.pad(x, (0, self.kernel_dim - d)) if d != self.kernel_dim else x

    def _append_hip(self, k: Tensor, v: Tensor, append_lens: Tensor) -> None:
        from .ops import hip_ext
        hip_ext.require().paged_kv_append(
            self._pad(k).to(torch.bfloat16).contiguous(),
            self._pad(v).to(torch.bfloat16).contiguous(),
            self.k_pages, self.v_pages, self.k_scales, self.v_scales,
            self.block_table, self.seq_lens, append_lens)

    def _append_eager(self, k: Tensor, v: Tensor, lens: list[int]) -> None:
        """CPU fallback: index_put of the new rows (quantize_kv_cache for
        fp8) at the same positions the append kernel writes."""
        ps = self.page_size
        pg_idx, row_idx, src_b, src_t = [], [], [], []
        for s, n_new in enumerate(lens):
            for t in range(n_new):
                pos = self._lens[s] + t
                pg_idx.append(self._pages[s][pos // ps])
                row_idx.append(pos % ps)
                src_b.append(s)
                src_t.append(t)
        pg_idx = torch.tensor(pg_idx, dtype=torch.long)
        row_idx = torch.tensor(row_idx, dtype=torch.long)
        # (tokens, hk, D) rows in pool order
        kb = self._pad(k).to(torch.bfloat16)[src_b, :, src_t]
        vb = self._pad(v).to(torch.bfloat16)[src_b, :, src_t]
        if self.fp8:
            from .ops.fp8 import quantize_kv_cache
            k8, v8, ks, vs = quantize_kv_cache(kb, vb)
            self.k_pages[pg_idx, :, row_idx] = k8
            self.v_pages[pg_idx, :, row_idx] = v8
            self.k_scales[pg_idx, :, row_idx] = ks
            self.v_scales[pg_idx, :, row_idx] = vs
        else:
            self.k_pages[pg_idx, :, row_idx] = kb
            self.v_pages[pg_idx, :, row_idx] = vb

    def release_prefix(self, keep_from) -> int:
        """Free the pages a lookback window has left behind.

        `keep_from` is a host list (or int tensor, read on the host like
        `append`'s lens) with one position per sequence: "no later call
        attends keys below this".  Every page of sequence s whose rows all
        lie below min(keep_from[s], seq_len) goes back to the free list and
        its table slot is set to -1 (one index_copy_, like `append`'s new
        pages); nothing is read from the device.  host_starts[s] becomes the
        number of released tokens: a multiple of page_size that never
        decreases and never exceeds keep_from[s].  Releasing the same prefix
        again does nothing.  Returns the number of pages freed.

        The table stays indexed by absolute position (no ring indexing):
        released slots are not reused and max_pages_per_seq still bounds the
        absolute length of a sequence.
        """
        if isinstance(keep_from, Tensor):
            keep_from = keep_from.tolist()
        keep = [int(x) for x in keep_from]
        if len(keep) != self.max_seqs:
            raise ValueError(f"release_prefix: keep_from has {len(keep)} entries, "
                             f"the cache holds {self.max_seqs} sequences")
        if any(x < 0 for x in keep):
            raise ValueError("release_prefix: keep_from must be >= 0")
        ps = self.page_size
        flat_idx = []
        for s in range(self.max_seqs):
            start = min(keep[s], self._lens[s]) // ps * ps
            for slot in range(self._starts[s] // ps, start // ps):
                self._free.append(self._pages[s][slot])
                self._pages[s][slot] = -1
                flat_idx.append(s * self.max_pages_per_seq + slot)
            self._starts[s] = max(self._starts[s], start)
        if flat_idx:
            self.block_table.view(-1).index_copy_(
                0, torch.tensor(flat_idx, dtype=torch.long).to(self.device),
                torch.full((len(flat_idx),), -1, dtype=torch.int32).to(self.device))
        return len(flat_idx)

    def check_released(self, name: str, lows) -> None:
        """Host-side guard of the attention entry points, from the mirrors
        alone and before any launch.  lows[s] is the smallest key position the
        call attends in sequence s (None: it attends nothing there), or
        `lows` itself is None when the call has no window.  Raises ValueError
        if a sequence with released pages would be read below host_starts."""
        for s, start in enumerate(self._starts):
            if start == 0:
                continue
            if lows is None:
                raise ValueError(
                    f"{name}: sequence {s} has released its first {start} keys "
                    f"(release_prefix); pass the window they were released for")
            if lows[s] is not None and lows[s] < start:
                raise ValueError(
                    f"{name}: sequence {s} would attend from key {lows[s]}, but "
                    f"keys below {start} are released (release_prefix)")

    def free(self, seq: int) -> None:
        """Return the pages sequence `seq` still holds to the pool and zero
        its length and its released prefix."""
        self._free.extend(pg for pg in reversed(self._pages[seq]) if pg >= 0)
        self._pages[seq] = []
        self._lens[seq] = 0
        self._starts[seq] = 0
        self.block_table[seq].fill_(-1)
        self.seq_lens[seq].fill_(0)

    # ---- read-back (debugging / tests) ----------------------------------
    def gather(self, seq: int) -> tuple[Tensor, Tensor]:
        """Dense (k, v), each (hk, seq_len, dim_head), of one sequence:
        bf16 as stored, or fp32 dequantised for an fp8 cache.  Rows below
        host_starts[seq] (released pages) come back as zeros, so positions
        stay absolute."""
        n = self._lens[seq]
        gone = self._starts[seq] // self.page_size
        pages = torch.tensor([max(pg, 0) for pg in self._pages[seq]],
                             dtype=torch.long).to(self.device)

        def dense(pool, scales):
            x = pool[pages]                                   # (np, hk, ps, D)
            if self.fp8:
                x = (x.view(torch.float8_e4m3fn).float()
                     * torch.exp2(scales[pages].float() - 127.0).unsqueeze(-1))
            if gone:
                x[:gone] = 0
            x = x.permute(1, 0, 2, 3).reshape(self.kv_heads, -1, self.kernel_dim)
            return x[:, :n, :self.dim_head].contiguous()

        return dense(self.k_pages, self.k_scales), dense(self.v_pages, self.v_scales)
