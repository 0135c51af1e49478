// Body of the paged row decode kernels (decode_paged.hip), included once per
// kernel with D, FP8, WIN and SOFTCLAMP in scope and `p` the kernel's
// PagedDecodeParams.  It is text, not a function: moved into an always_inline
// function, the instantiations without the clamp lose the instruction stream
// they had (the grid-size reads are lowered differently).

    // one wave per (b, q-head, query token); 4 waves per block; grid.y is
    // the kv-split.  The wave->row mapping (decode_row) and the row body
    // (DecodeState) are decode_common.h's, shared with the dense kernels.
    const int rows = p.b * p.h * p.nq;
    // grid = (row blocks, S) like the dense kernels.  With ragged lengths the
    // hardware's round-robin of consecutive workgroup ids over the 8 XCDs
    // would pin each sequence's row blocks (blockIdx.x, the fast index) to
    // the same one or two XCDs — the longest sequence then streams through a
    // fraction of the chip (measured: ragged b=8 601 us vs 241 us).
    // chunk_major (set by the binding for b > 1) re-reads the linear
    // workgroup id with the kv chunk as the fast index, so every row's
    // chunks spread over all XCDs.
    const unsigned lin = blockIdx.x + gridDim.x * blockIdx.y;
    const int row_block = p.chunk_major ? (int)(lin / gridDim.y) : (int)blockIdx.x;
    const int chunk = p.chunk_major ? (int)(lin % gridDim.y) : (int)blockIdx.y;
    const int wave_global = (row_block * 4) + (threadIdx.x >> 6);
    if (wave_global >= rows) return;
    const DecodeRow r = decode_row(wave_global, p.h, p.hk, p.nq);
    const int b = r.b, hk = r.hk, iq = r.iq;
    const int lane = threadIdx.x & 63;

    // per-row key limit: the sequence's own length (never past what the
    // table can address); with `causal` the last nq cached positions are the
    // queries' own tokens and query iq sees up to and including its own
    const int shift = p.page_shift;
    const long cap = (long)p.max_pages << shift;
    long limit = min((long)p.seq_lens[b], cap);
    if (p.causal) limit -= (p.nq - 1 - iq);
    limit = max(limit, 0L);
    // lookback window (WIN): the row's query sits at position
    // seq_len + kv_after - nq + iq in local key coordinates (kv_after =
    // tokens of the sequence held by later ranks) and attends only keys
    // j >= position - win, so its span is [lo, limit).  The unwindowed
    // instantiation keeps lo = base = 0 as constants.
    long lo = 0;
    if constexpr (WIN) {
        const long len = min((long)p.seq_lens[b], cap);
        const long after = p.kv_after ? (long)p.kv_after[b] : 0L;
        lo = min(max(len + after - p.nq + iq - p.win, 0L), limit);
    }
    const long base = lo & ~63L;
    // kv-split of THIS row's span: a slice of the batch-wide max range
    // would leave short sequences on chunk 0 only.  The span is cut from
    // its 64-aligned start and the per-chunk length is rounded up to 64 keys
    // so every loop pass of the wave starts 64-aligned (for page_size >= 64
    // its 64 keys then share one page).  Chunks past the row's end are
    // empty and still write their partial below; so does a row whose span
    // is empty (lo == limit), which touches neither the table nor the pool.
    long per = (limit - base + gridDim.y - 1) / gridDim.y;
    per = (per + 63) & ~63L;
    const long j_lo = base + chunk * per;
    const long j_hi = (!WIN || lo < limit) ? min(limit, j_lo + per) : j_lo;

    const int* bt = p.block_table + (long)b * p.max_pages;
    const long pmask = (1L << shift) - 1;
    const bool uniform_page = shift >= 6;

    const float c = p.softclamp_value;
    const float rcp_c = SOFTCLAMP ? __builtin_amdgcn_rcpf(c) : 0.f;

    DecodeState<D> st;
    st.init((const __bf16*)p.q + ((long)r.bh * p.nq + iq) * D);

    // each lane handles keys lane, lane+64, ...; the page id of the NEXT pass
    // is fetched before the current rows are consumed so the dependent
    // table -> row load chain overlaps the row math.  Table entries are read
    // only for j < limit, i.e. only valid entries are ever touched.
    // Keys in [base, lo) fall in the row's FIRST pass only (every later pass
    // starts at or beyond base + 64 > lo) and do no row math.  Their table
    // entries differ by page size:
    //   page_size < 64  such a key can sit in a released page (entry -1):
    //                   a lane reads its entry only when lo <= j;
    //   page_size >= 64 the pass lies in the page that holds lo, which the
    //                   host guard keeps live, and the id comes from the
    //                   first lane: the read is NOT predicated on lo (lane 0
    //                   would otherwise hand -1 to the whole wave) and only
    //                   the row math is masked.
    long j = j_lo + lane;
    int pg = (j < j_hi && (!WIN || uniform_page || j >= lo)) ? bt[j >> shift] : -1;
    while (j < j_hi) {
        const long jn = j + 64;
        const int pg_next = jn < j_hi ? bt[jn >> shift] : -1;
        // page_size >= 64: the wave's 64 keys share the page -> scalar id
        if (uniform_page) pg = __builtin_amdgcn_readfirstlane(pg);
        // a page id outside the pool is never dereferenced
        if ((unsigned)pg < (unsigned)p.num_pages && (!WIN || j >= lo)) {
            const long row = ((((long)pg * p.hk + hk) << shift) | (j & pmask));
            if constexpr (FP8) {
                st.template fold_fp8<SOFTCLAMP>((const unsigned char*)p.k_pages + row * D,
                                                (const unsigned char*)p.v_pages + row * D,
                                                (const unsigned char*)p.kscale + row,
                                                (const unsigned char*)p.vscale + row,
                                                p.scale, c, rcp_c);
            } else {
                st.template fold_bf16<SOFTCLAMP>((const __bf16*)p.k_pages + row * D,
                                                 (const __bf16*)p.v_pages + row * D,
                                                 p.scale, c, rcp_c);
            }
        }
        j = jn;
        pg = pg_next;
    }

    // an empty chunk still writes its partial (out = 0, lse = MASK_VALUE_F)
    const long slot = (long)chunk * rows + (long)r.bh * p.nq + iq;
    st.finish(lane, p.out + slot * D, p.lse + slot);
