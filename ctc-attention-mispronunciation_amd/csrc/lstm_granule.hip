// Persistent BiLSTM layer kernel, split-bf16 arithmetic: the whole recurrence of one BiLSTM layer in ONE launch (lstm_layer_granule_kernel below).
// The per-step launches (lstm_step.hip) re-read W_hh (4.7 MB) from L2 every step; measured, a CU ingests only ~50-100 GB/s from L2, so at
// fused batch sizes the step is bound by that re-read.  The persistent form keeps every workgroup's W_hh rows in registers for
// the whole layer and moves only h between the workgroups of a team.  (An earlier form of it -- 16-workgroup teams around a
// per-team arrival counter -- was superseded by the data-tagged hand-off and is no longer built.)
#include "lstm_granule.h"
#include "lstm_host.h"

namespace mdd {

// ---- persistent layer kernel, data-tagged hand-off ("the data IS the flag", Guideline 16 form R2).  Same team structure, but (1) a team is 8
// workgroups (32 teams = 2 directions x 16 batch groups), each workgroup owning 4H/8 gate rows: RTW row tiles per wave, fragments resident in
// registers; the panel a workgroup pulls per step is half as tall; (2) h travels as 16-byte chunks of FOUR units of one batch row, {hi0 hi1 hi2 hi3 |
// lo0 lo1 lo2 lo3}, whose epoch tag (1..3 = step % 3 + 1) rides in the spare last bits of the lo halves (split_h clears them: bit 0 of the tag in the
// even units, bit 1 in the odd ones): the producer just stores them write-through -- no drain, no barrier, no counter -- and the consumer checks the
// tags of what it fetched ("the data IS the flag").  A chunk is one lane's single 16-byte store, so a chunk is either old or new as a whole.  One L2
// round trip replaces three (drain, counter add, poll).  A panel of one parity only ever holds step s or step s-2 (nobody publishes step s before
// everyone has read s-2), whose tags differ; the exchange buffer is zeroed before every launch (tag 0 is never valid), so replays cannot see a
// previous launch's data.  The hand-off is bound by the bytes all 256 workgroups pull past their L2s and by the ~2 us a write-through store takes to
// become visible, hence the dense format (4 bytes per unit and row) and the chunk order = (unit / 4) * 16 + row: a workgroup's share is one
// contiguous run, the sweep a linear LDS-DMA copy, and the chunks are the MFMA operands as they lie (see the kernel body).
// A team's batch rows come in NBT tiles of 16 (one MFMA column tile each).  The tiles are independent recurrences and are advanced in turn, each with
// its own panel and epoch: while one tile's h_s travels to the team (the hand-off is ~2 us of pure latency), the workgroup runs the other tiles'
// MFMAs and cell updates.  With three or more tiles a tile's panel has been complete for a whole phase when its turn comes, so its sweep is requested
// one phase AHEAD (LDS-DMA into the other panel buffer, one piece per k-step of the MFMA loop); with two tiles it is requested after the MFMAs of the
// phase before (the panel is not complete earlier); with one there is nothing to overlap.  The gate pre-activations never occupy registers: each
// tile's next [16 rows x 4*UW] slab is fetched by LDS-DMA as soon as the cell update has consumed the current one.
template <int H, int NBT, int RTW, bool TRAIN = false>
__global__ __launch_bounds__(256, 1) void lstm_layer_granule_kernel(PersistArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int NTH = 256, KS = H / 32, RM = 4 * H / 8;
    constexpr int PF = NBT == 1 ? 0 : (NBT == 2 ? 1 : 2);          // where the next phase's sweep is requested (see above)
    static_assert(RM == 4 * RTW * 16, "4 waves x RTW row tiles must cover the workgroup's gate rows");
    constexpr int UW = RM / 4;                                      // units this workgroup owns (a 2*UW-byte run per output row and plane)
    unsigned short *Oh = reinterpret_cast<unsigned short *>(smem), *Ol = Oh + 16 * UW;   // step outputs, [row][unit]
    float *Of = reinterpret_cast<float *>(Ol + 16 * UW);
    unsigned int *Og = reinterpret_cast<unsigned int *>(Of + 16 * UW);   // this step's h as tagged words, [unit chunk][row][4 units]: the publish order
    float *Gx = reinterpret_cast<float *>(Og + 16 * UW);            // [NBT][2 step parities][16 rows][UW units][4 gates] gate pre-activations (LDS-DMA)
    constexpr int GXT = 16 * UW * 4;                                // floats per tile slab
    constexpr int PANB = 16 * H * 4;                                // bytes of one tile panel
    unsigned char *Rw = reinterpret_cast<unsigned char *>(Gx + NBT * 2 * GXT);   // [2][PANB] tile panels as they travel (LDS-DMA), alternating per phase
    static_assert(UW % 8 == 0 && (16 * UW) % NTH == 0, "output rows are whole 16-byte chunks; the gx slab is whole 1 KB wave loads");
    __shared__ int s_fail;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, kq = lane >> 4;
    const Team8 tm = team8_of_block();
    const int team = tm.team, member = tm.member, d = tm.d, g = tm.g;
    const int B = a.B, T = a.T;
    if (tid == 0) s_fail = 0;

    bf16x8 ah[RTW][KS], al[RTW][KS];
    float osc[RTW], osh[RTW];
#pragma unroll
    for (int rt = 0; rt < RTW; rt++) {
        const int r0 = member * RM + (wave * RTW + rt) * 16;
        const int unit = (r0 >> 2) + kq;
        osc[rt] = a.oscale ? a.oscale[d * H + unit] : 1.f;
        osh[rt] = a.oscale ? a.oshift[d * H + unit] : 0.f;
        const unsigned short *wh = a.whh.hi + ((size_t)d * 4 * H + r0 + li) * H + kq * 8;
        const unsigned short *wl = a.whh.lo + ((size_t)d * 4 * H + r0 + li) * H + kq * 8;
#pragma unroll
        for (int ks = 0; ks < KS; ks++) {
            ah[rt][ks] = *reinterpret_cast<const bf16x8 *>(wh + ks * 32);
            al[rt][ks] = *reinterpret_cast<const bf16x8 *>(wl + ks * 32);
        }
    }
    float cst[RTW][NBT];
#pragma unroll
    for (int rt = 0; rt < RTW; rt++)
#pragma unroll
        for (int bt = 0; bt < NBT; bt++) cst[rt][bt] = 0.f;
    int slen[NBT];                                                  // steps valid for this lane's batch row of tile bt (fused batches of different lengths)
#pragma unroll
    for (int bt = 0; bt < NBT; bt++) {
        const int lb = bt * 16 + li, row = g * a.BGr + lb;
        slen[bt] = (a.seqlen && lb < a.BGr && row < B) ? a.seqlen[row] : T;
    }
    // A tile panel in the exchange buffer and in LDS: 16-byte chunks {4 tagged words = 4 consecutive units of one row},
    // chunk index = (unit / 4) * 16 + row.  A workgroup's share (its UW units x 16 rows) is then ONE contiguous run, the
    // sweep is a linear copy, and the MFMA operand of lane (row li, k-quarter kq) at k-step ks is the two chunks
    // (ks * 8 + kq * 2 + {0, 1}) * 16 + li: the 16 lanes of a quarter read 256 contiguous bytes (no bank conflicts).
    constexpr size_t tgran = (size_t)16 * H / 2;                   // 8-byte granules per tile panel
    const size_t pgran = NBT * tgran;                              // granules per (parity, team)
    constexpr int NLD = 16 * H / 4 / NTH;                          // 16-byte chunks per thread and tile
    static_assert(16 * H / 4 % NTH == 0 && H % 32 == 0, "panel must be whole passes of the workgroup");
    u64 *hxg = reinterpret_cast<u64 *>(a.hx);
    unsigned int *abortf = a.sync + kPersistAbortWord;
    long long ph[6] = {0, 0, 0, 0, 0, 0}, tst = a.dbg ? (long long)__builtin_readcyclecounter() : 0;

    // gate pre-activations of (tile bt, time tt) -> Gx[bt]: one LDS-DMA piece per row tile of the wave, and lane (row li,
    // unit kq) of piece rt fetches exactly the 16 bytes (i, f, g, o of its unit and row) that the same lane consumes in
    // the cell update of row tile rt: nothing crosses waves, so no barrier stands between the transfer and its use
    constexpr int NGX = RTW;                                        // 1 KB wave loads per slab and wave
    const unsigned gvoff = (unsigned)(d * 4 * H + (member * UW + wave * RTW * 4 + kq) * 4) * 4u;   // byte offset of row tile 0's unit in a gx row
    const unsigned wave_lds = __builtin_amdgcn_readfirstlane((unsigned)wave * 1024u);   // a wave's 1 KB slot inside a 4 KB LDS-DMA pass
    const unsigned wave_gx = __builtin_amdgcn_readfirstlane((unsigned)wave * (unsigned)(RTW * 1024));   // a wave's RTW row tiles inside a slab
    const unsigned gx_lds = (unsigned)(unsigned long long)(lds_void_t *)Gx, rw_lds = (unsigned)(unsigned long long)(lds_void_t *)Rw;
    const Team8Dma q = {hxg, pgran, B, g, li, team, tid, gvoff, wave_lds, wave_gx, gx_lds, rw_lds};
    auto load_gx = [&](int bt, int par, int tt, int i0 = 0, int i1 = 99) { team8_load_gx<H>(a, q, bt, par, tt, i0, i1); };
    // Layer outputs and the publish are read back from the LDS tiles as 16- or 8-byte pieces and leave as buffer stores.  Every wave stores exactly
    // the units it produced (its RTW row tiles = 4*RTW consecutive units of all 16 rows): the tiles never cross waves, so no barrier stands between
    // the cell update and the stores either.  Every wave issues a fixed number of store instructions per destination (lanes without a piece, and
    // nothing else, are dropped by the buffer range check; lanes of rows past the batch repeat the tile's last valid row: identical bytes to the same
    // address), so that the number of memory operations a wave issues after a sweep request is known exactly -- see the counted wait below.  The LDS
    // reads of a phase are issued together, ahead of the stores.
    constexpr int UWW = UW / 4, PCW = UWW / 4;                          // units per wave; 4-unit pieces per row (16 B of fp32, 8 B of a bf16 plane)
    constexpr int PWR = 16 * PCW, PWP = 16 * (UW / 4) / 4;               // pieces per wave: layer outputs (per destination), publish chunks
    static_assert(UWW % 4 == 0 && PWR <= 64 && PWP == 16 * RTW, "a wave's output pieces fit one instruction; it publishes its own row tiles");
    const int orow = lane / PCW, ocol = wave * UWW + (lane - orow * PCW) * 4;   // output role of this lane: tile row, first of its 4 units
    const int qp = min(wave * PWP + lane, 16 * (UW / 4) - 1);
    const unsigned offp = lane < PWP ? (unsigned)(member * 16 * (UW / 4) + wave * PWP + lane) * 16u : 0xffffffffu;
    const size_t slab = (size_t)B * 2 * H;                              // elements of one time step of the layer output
    auto tile_rows = [&](int bt) { const int nv = min(a.BGr, B - g * a.BGr) - bt * 16; return nv < 0 ? 0 : (nv > 16 ? 16 : nv); };
    struct OutRegs { u32x2 vh, vl; u32x4 vr; int r; };
    auto out_read = [&](int bt, OutRegs &o) {
        o.r = min(orow, max(tile_rows(bt), 1) - 1);
        if (a.out_split.hi) {
            o.vh = *reinterpret_cast<const u32x2 *>(Oh + o.r * UW + ocol);
            o.vl = *reinterpret_cast<const u32x2 *>(Ol + o.r * UW + ocol);
        }
        if (a.out_raw) o.vr = *reinterpret_cast<const u32x4 *>(Of + o.r * UW + ocol);
    };
    auto out_write = [&](int bt, int tt, const OutRegs &o) -> int {
        if (tile_rows(bt) == 0) return 0;
        int issued = 0;
        const unsigned el = lane < PWR ? (unsigned)((g * a.BGr + bt * 16 + o.r) * 2 * H + d * H + member * UW + ocol) : 0x3fffffffu;   // element offset in the step's slab (out of range: dropped)
        if (a.out_split.hi) {
            const __amdgpu_buffer_rsrc_t rh = __builtin_amdgcn_make_buffer_rsrc(a.out_split.hi + (size_t)tt * slab, 0, (int)(slab * 2), 0x00020000);
            const __amdgpu_buffer_rsrc_t rl = __builtin_amdgcn_make_buffer_rsrc(a.out_split.lo + (size_t)tt * slab, 0, (int)(slab * 2), 0x00020000);
            __builtin_amdgcn_raw_buffer_store_b64(o.vh, rh, el * 2u, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b64(o.vl, rl, el * 2u, 0, 0);
            issued += 2;
        }
        if (a.out_raw) {
            const __amdgpu_buffer_rsrc_t rs_ = __builtin_amdgcn_make_buffer_rsrc(a.out_raw + (size_t)tt * slab, 0, (int)(slab * 4), 0x00020000);
            __builtin_amdgcn_raw_buffer_store_b128(o.vr, rs_, el * 4u, 0, 0);
            issued++;
        }
        return issued;
    };
    auto store_out = [&](int bt, int tt) -> int { OutRegs o; out_read(bt, o); return out_write(bt, tt, o); };
    // Sweep request of (tile bt, step s) into panel buffer pb: a linear LDS-DMA copy of the tile's panel (parity (s-1)&1), NLD pieces per wave.  With
    // two or more tiles it is issued a phase ahead; it is waited for with vmcnt(K), K = the exact number of memory instructions this wave has issued
    // since (the wave's memory counter is in-order: vmcnt(0) would also wait for the acknowledgement of every store issued after the request -- the
    // write-through publish alone takes ~1 us).
    auto request_sweep = [&](int bt, int s, int pb, int i0 = 0, int i1 = 99) { team8_request_sweep<H>(q, bt, (s - 1) & 1, pb, i0, i1); };
#pragma unroll
    for (int bt = 0; bt < NBT; bt++) load_gx(bt, 0, d ? (T - 1) : 0);
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0), compiler-visible: the weight fragments are in registers from here on (no waits for them inside the loop)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    lds_barrier();

    int pend_bt = -1, pend_t = 0;                                   // PF == 0: the phase whose outputs still sit in the LDS tiles
    bool requested = false;                                         // the panel of the phase about to start is in flight / staged
    int younger = 0, early_gx = 0;                                  // memory instructions this wave issued after that request
    int pc = 0;                                                     // phases with a sweep so far: panel buffer = pc & 1
    for (int s = 0; s < T; s++) {
        const int t = d ? (T - 1 - s) : s;
#pragma unroll
        for (int bt = 0; bt < NBT; bt++) {
            const int nbt = bt + 1 < NBT ? bt + 1 : 0, ns = bt + 1 < NBT ? s : s + 1;     // the next phase
            f32x4 acc[RTW];
#pragma unroll
            for (int rt = 0; rt < RTW; rt++) acc[rt] = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (s > 0) {
                const int pb = pc & 1;
                ++pc;
                const unsigned ep = (unsigned)((s - 1) % 3 + 1), etag = (ep & 1u) | ((ep >> 1) << 16);   // tag of step s-1: bit 0 in lo0, bit 1 in lo1
                long long t0 = 0;   // wall clock at the first retry (read lazily: its scalar load would sit in front of every phase's first barrier)
                // ---- the tile's panel of step s-1 -> LDS
                if (PF == 0) {
                    // one tile: nothing to overlap.  Each wave polls its own pieces (read back through LDS) until all tags match.
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // own publish acknowledged: a request sent earlier only finds stale tags
                    request_sweep(bt, s, pb);
                    wait_vmcnt(pend_bt >= 0 ? store_out(pend_bt, pend_t) : 0);   // the previous phase's outputs, behind the sweep in the queue
                    int polls = 0;
                    while (true) {
                        unsigned bad = 0;
#pragma unroll
                        for (int i = 0; i < NLD; i++) {
                            const u32x4 v = *reinterpret_cast<const u32x4 *>(Rw + (size_t)pb * PANB + (size_t)(i * NTH + tid) * 16);
                            bad |= (v[2] ^ etag) | (v[3] ^ etag);
                        }
                        ++polls;
                        if (!__any((bad & 0x00010001u) != 0)) break;
                        if ((polls & 63) == 0) {
                            int ab = 0;
                            if (t0 == 0) t0 = wall_clock64();
                            if (lane == 0) ab = (__hip_atomic_load(abortf, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) || (wall_clock64() - t0 > kPersistStallTicks);
                            if (__any(ab)) {
                                if (lane == 0) { __hip_atomic_store(abortf, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); atomicExch(a.err_flag, 2); s_fail = 1; }
                                break;
                            }
                        }
                        request_sweep(bt, s, pb);
                        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    }
                    if (a.dbg) ph[5] += polls;
                } else {
                    // requested a phase ago (or just now: the first step after s = 0)
                    if (!requested) { request_sweep(bt, s, pb); younger = 0; }
                    const long long tw = a.dbg ? (long long)__builtin_readcyclecounter() : 0;
                    wait_vmcnt(younger);
                    if (a.dbg) ph[1] += (long long)__builtin_readcyclecounter() - tw;
                }
                requested = false;
                lds_barrier();                                          // every wave's pieces of the panel are in LDS
                PSTAMP(0);
                if (s_fail) return;
                // The LDS-DMA pieces of this phase -- this tile's next gx slab (other parity buffer), then, with three or more
                // tiles, the next tile's sweep (its panel was published a whole phase ago) -- are issued one per k-step inside
                // the MFMA loop: a piece costs the wave ~100 cycles of issue, which the MFMAs in flight cover.  The slab goes
                // first: nothing slow may be younger than the sweep request (see the counted wait at its consumption).
                const bool early = PF != 0 && a.early && ns < T;
                if (early) { request_sweep(nbt, ns, pb ^ 1); requested = true; }
                const bool do_rq = PF == 2 && ns < T && !early;
                const int tt_next = d ? max(T - 2 - s, 0) : min(s + 1, T - 1);   // the step whose slab this phase requests
                // The MFMA operands come straight from the travelling chunks (no unpacking pass, no second copy in LDS): per k-step two 16-byte
                // chunks {hi x4 | lo' x4} -> the hi halves of both are one operand, the lo halves (tag bits cleared: 4 v_and) the other.  One tagged
                // word per chunk is summed on the way (bit 0 and bit 16 fields; 2*KS words per lane cannot overflow a field).  With two or more tiles
                // the panel was requested ahead and is used unchecked: if the sum is off, some member's h had not landed when the request was served;
                // every wave sees the same panel, so all take the same decision: request it again and redo the tile's products (not seen with the
                // request placed after the MFMAs: it trails the publish by ~2 us).
                const unsigned char *fb = Rw + (size_t)pb * PANB + kq * 512 + li * 16;
                int tries = 0;
                while (true) {
                    constexpr int PD = 3;                             // chunk pairs read ahead of their use
                    u32x4 ra[PD], rb[PD];
#pragma unroll
                    for (int p = 0; p < PD; p++) {
                        ra[p] = *reinterpret_cast<const u32x4 *>(fb + p * 2048);
                        rb[p] = *reinterpret_cast<const u32x4 *>(fb + p * 2048 + 256);
                    }
                    unsigned sraw = 0, smask = 0;                     // sums of the lo words with / without their tag bits
                    MDD_SCHED_HINT();
#pragma unroll
                    for (int ks = 0; ks < KS; ks++) {
                        const u32x4 xa = ra[ks % PD], xb = rb[ks % PD];
                        if (ks + PD < KS) {
                            ra[ks % PD] = *reinterpret_cast<const u32x4 *>(fb + (ks + PD) * 2048);
                            rb[ks % PD] = *reinterpret_cast<const u32x4 *>(fb + (ks + PD) * 2048 + 256);
                        }
                        u32x4 hq, lq;
                        hq[0] = xa[0]; hq[1] = xa[1]; hq[2] = xb[0]; hq[3] = xb[1];
                        lq[0] = xa[2] & 0xfffefffeu; lq[1] = xa[3] & 0xfffefffeu; lq[2] = xb[2] & 0xfffefffeu; lq[3] = xb[3] & 0xfffefffeu;
                        if (PF != 0) { sraw += xa[2] + xb[2]; smask += lq[0] + lq[2]; }   // one tagged word per 16-byte chunk: a chunk is one lane's single store
                        bf16x8 bh = __builtin_bit_cast(bf16x8, hq), bl = __builtin_bit_cast(bf16x8, lq);
                        // The slab pieces are issued unconditionally (a branch per k-step costs the loop more than the piece: -2.6 % on the
                        // product section): at the last step they fetch a valid slab nobody reads, in a redo they fetch the same slab again.
                        // (Round 2 kept a guard around them in the three- and four-tile forms because lifting it changed last bits there: that
                        // was the hidden-hazard class described at mfma_v() -- another code shape, another schedule around the asm MFMA --
                        // not the request itself; with the hazards expressed the bits stay.)  The sweep pieces of the three- and four-tile
                        // forms stay conditional: after a redo, or with no next phase, there is nothing to request.
                        if (ks < NGX) load_gx(bt, (s + 1) & 1, tt_next, ks, ks + 1);
                        else if (PF == 2 && tries == 0 && ks < NGX + NLD) { if (do_rq) request_sweep(nbt, ns, pb ^ 1, ks - NGX, ks - NGX + 1); }
                        // product-major order: consecutive MFMAs hit different accumulators (no dependent-issue stall);
                        // each accumulator still sees ah.bl, al.bh, ah.bh in that order (bit-identical to the step kernel)
                        // (the scheduler would otherwise regroup them per accumulator into dependent back-to-back pairs)
                        bf16x8 ak[RTW];
#pragma unroll
                        for (int rt = 0; rt < RTW; rt++) ak[rt] = ah[rt][ks];
                        mfma_operands_ready(bh, bl, ak);
#pragma unroll
                        for (int rt = 0; rt < RTW; rt++) {   // the first product of a tile starts from a literal zero: no accumulator clearing per phase (or per redo)
                            if (ks == 0) mfma_v0(acc[rt], ak[rt], bl); else mfma_v(acc[rt], ak[rt], bl);
                        }
                        MDD_SCHED_HINT();
#pragma unroll
                        for (int rt = 0; rt < RTW; rt++) mfma_a(acc[rt], al[rt][ks], bh);   // lo fragments stay in AGPRs and feed the MFMA from there
                        MDD_SCHED_HINT();
#pragma unroll
                        for (int rt = 0; rt < RTW; rt++) mfma_v(acc[rt], ak[rt], bh);
                        MDD_SCHED_HINT();
                    }
                    const unsigned tsum = sraw - smask;
                    static_assert(NGX + NLD <= KS, "one LDS-DMA piece per k-step");
                    if (PF == 0 || !__any(tsum != (unsigned)(2 * KS) * etag)) break;
                    // ---- stale panel (identical verdict in every wave): fetch it again, redo the products
                    ++tries;
                    if (a.dbg) ph[5] += 1;
                    if (t0 == 0) t0 = wall_clock64();
                    if (lane == 0 && ((__hip_atomic_load(abortf, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) || (wall_clock64() - t0 > kPersistStallTicks))) {
                        __hip_atomic_store(abortf, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); atomicExch(a.err_flag, 2); s_fail = 1;
                    }
                    lds_barrier();                                      // every wave is done reading the panel; s_fail is visible
                    if (s_fail) return;
                    request_sweep(bt, s, pb);
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    lds_barrier();
                }
                if (a.dbg && PF != 0) ph[5] += 1;
                if (do_rq) requested = true;
                int in_flight = NGX + (PF != 2 ? ((early && !tries) ? NLD : 0)      // (a redo's vmcnt(0) came before its own slab pieces)
                                               : ((!tries && (do_rq || early)) ? NLD : 0));
                early_gx = (early && !tries) ? NGX : 0;                             // memory instructions younger than an early request
                if (PF == 1 && ns < T && !early) {   // two tiles: the other tile's panel has had the length of these MFMAs to arrive
                    request_sweep(nbt, ns, pb ^ 1); requested = true;
                    in_flight += NLD;
                }
                wait_vmcnt(in_flight);   // everything older than this phase's pieces has landed: in particular this wave's part of the tile's current gx slab
            }
            if (s == 0 && T > 1) load_gx(bt, 1, d ? (T - 2) : 1);
            PSTAMP(2);
            // ---- cell update; h_s goes to the LDS tiles (outputs, and tagged words for the team)
            const unsigned tg = (unsigned)(s % 3 + 1);
            const int lb = bt * 16 + li;
            const bool valid = lb < a.BGr && g * a.BGr + lb < B;
            float4 gv[RTW];
            float hn[RTW];
            mfma_drain();                        // (the asm MFMAs' results are read by vector instructions from here on)
#pragma unroll
            for (int rt = 0; rt < RTW; rt++)     // the slab reads together (one LDS round trip), each lane its own 16 bytes
                gv[rt] = *reinterpret_cast<const float4 *>(Gx + (bt * 2 + (s & 1)) * GXT + ((wave * RTW + rt) * 64 + lane) * 4);
#pragma unroll
            for (int rt = 0; rt < RTW; rt++) {   // branch-free: the row tiles' chains interleave
                const float ig = fast_sigmoid(acc[rt][0] + gv[rt].x), fg = fast_sigmoid(acc[rt][1] + gv[rt].y);
                const float cg = fast_tanh(acc[rt][2] + gv[rt].z), og = fast_sigmoid(acc[rt][3] + gv[rt].w);
                const bool live = !(d && t >= slen[bt]);              // the reverse direction starts at the row's own last step, from a zero state
                const float cn = fg * cst[rt][bt] + ig * cg;
                const float hr = og * fast_tanh(cn);
                hn[rt] = (valid && live) ? hr : 0.f;
                cst[rt][bt] = live ? cn : 0.f;
                if (TRAIN) {   // what the backward step reads: the gates after their nonlinearities and c_t, in the training layout (one 64-byte run per row and quad)
                    const unsigned el = valid ? (unsigned)(((g * a.BGr + lb) * 2 + d) * H + member * UW + (wave * RTW + rt) * 4 + kq) : 0x0fffffffu;
                    const __amdgpu_buffer_rsrc_t rg = __builtin_amdgcn_make_buffer_rsrc(a.gates_save + (size_t)t * B * 2 * H * 4, 0, B * 2 * H * 16, 0x00020000);
                    const __amdgpu_buffer_rsrc_t rc_ = __builtin_amdgcn_make_buffer_rsrc(a.c_save + (size_t)t * B * 2 * H, 0, B * 2 * H * 4, 0x00020000);
                    u32x4 gq;
                    gq[0] = __float_as_uint(ig); gq[1] = __float_as_uint(fg); gq[2] = __float_as_uint(cg); gq[3] = __float_as_uint(og);
                    __builtin_amdgcn_raw_buffer_store_b128(gq, rg, el * 16u, 0, 0);
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(cn), rc_, el * 4u, 0, 0);
                }
            }
#pragma unroll
            for (int rt = 0; rt < RTW; rt++) {
                const int cl = wave * RTW + rt, ul = cl * 4 + kq;        // chunk column and unit inside the workgroup's share
                const float ov = hn[rt] * osc[rt] + osh[rt];
                __bf16 ob = (__bf16)ov, ol = (__bf16)(ov - (float)ob);
                Oh[li * UW + ul] = *reinterpret_cast<unsigned short *>(&ob);
                Ol[li * UW + ul] = *reinterpret_cast<unsigned short *>(&ol);
                if (a.out_raw) Of[li * UW + ul] = hn[rt];
                const unsigned hw = split_h(hn[rt]);                   // chunk = {hi0 hi1 hi2 hi3 | lo0' lo1' lo2' lo3'}: tag bit 0 rides in the even units' lo, bit 1 in the odd units'
                unsigned short *ogp = reinterpret_cast<unsigned short *>(Og) + (cl * 16 + li) * 8 + kq;
                ogp[0] = (unsigned short)(hw & 0xffffu);
                ogp[4] = (unsigned short)((hw >> 16) | ((kq & 1) ? (tg >> 1) : (tg & 1u)));
            }
            PSTAMP(3);
            // ---- publish h_s (no drain, no signal): the workgroup's share of the tile's panel is one contiguous run of
            // 16 * UW / 4 chunks, written as 16-byte write-through stores straight from the Og tile (same order)
            younger = early_gx + (TRAIN ? 2 * RTW : 0); early_gx = 0;   // (TRAIN: the cell update's stores are younger than the sweep request too)
            {
                const bool pub = s + 1 < T, defer = PF == 0 && s > 0 && s + 1 < T;
                const u32x4 pv = *reinterpret_cast<const u32x4 *>(Og + qp * 4);
                OutRegs o;
                if (!defer) out_read(bt, o);
                if (pub) {   // all 16 rows of the tile (rows past the batch carry zeros and valid tags)
                    const __amdgpu_buffer_rsrc_t drs = __builtin_amdgcn_make_buffer_rsrc(hxg + (size_t)((s & 1) * 32 + team) * pgran + bt * tgran, 0, (int)(tgran * 8), 0x00020000);
                    __builtin_amdgcn_raw_buffer_store_b128(pv, drs, offp, 0, 16 /* sc1 */);
                    younger++;
                }
                // layer outputs: with one tile they wait for the next sweep's request (nothing else to hide them behind);
                // otherwise the next sweep is already in flight and they go out now
                if (defer) { pend_bt = bt; pend_t = t; }
                else { younger += out_write(bt, t, o); pend_bt = -1; }
            }
            if (s == 0) {   // no MFMA section with its barriers follows before these LDS regions are reused
                if (bt + 1 == NBT) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                lds_barrier();
            }
            PSTAMP(4);
        }
    }
    if (pend_bt >= 0) store_out(pend_bt, pend_t);
    if (a.dbg && tid == 0) for (int i = 0; i < 6; i++) a.dbg[blockIdx.x * 6 + i] = ph[i];
}

// The instantiations: {384, 256} x 1..4 tiles per team (training forward: 1..2), RTW = 4H / 8 / 64 row tiles per wave.  The stamps are a
// run-time branch of these kernels (PersistArgs::dbg), not instantiations of their own.
template <bool TRAIN> struct GranuleFamily : PersistFamily {
    using List = std::conditional_t<TRAIN, InstList<Inst<384, 1>, Inst<384, 2>, Inst<256, 1>, Inst<256, 2>>,
                                    InstList<Inst<384, 1>, Inst<384, 2>, Inst<384, 3>, Inst<384, 4>, Inst<256, 1>, Inst<256, 2>, Inst<256, 3>, Inst<256, 4>>>;
    template <int H, int N, bool> static auto kernel() { return lstm_layer_granule_kernel<H, N, H / 128, TRAIN>; }
    static constexpr size_t lds(int H, int N) { return team8_lds_bytes(H, N); }
};

int launch_lstm_layer_granule(const LstmStepArgs &s, unsigned short *hx, unsigned int *sync, int *err_flag, hipStream_t st,
                              long long *stamps, bool early) {
    PersistArgs a = persist_args(s, hx, sync, err_flag, stamps);
    a.whh = s.whh_split; a.out_split = s.out_split; a.early = early; a.gates_save = s.gates_save; a.c_save = s.c_save;
    if (a.out && a.out != a.out_raw) { set_error("granule lstm: a separate scaled fp32 output is not supported (split planes carry it)"); return MDD_ERR_ARG; }
    const int nbt = team8_tiles(s.B);
    const size_t live = team8_hx_live_bytes(s.H, nbt * 16);
    if (s.gates_save) {   // training forward: gates and cell states are saved for the backward pass (B <= 512)
        if (!s.c_save || a.seqlen || (size_t)s.B * 2 * s.H * 16 > 0x7fffffffu) { set_error("granule lstm (train): bad arguments"); return MDD_ERR_ARG; }
        const int rc = launch_instantiation<GranuleFamily<true>>(s.H, nbt, false, a, hx, live, sync, st);
        if (rc == kNoInstantiation) { set_error("granule lstm (train): built for H in {256,384}, B <= 512 (H=%d B=%d)", s.H, s.B); return MDD_ERR_ARG; }
        return rc;
    }
    if (nbt < 1 || nbt > kTeam8MaxTiles) { set_error("granule lstm: B=%d needs %d row tiles per team (max %d)", s.B, nbt, kTeam8MaxTiles); return MDD_ERR_ARG; }
    const int rc = launch_instantiation<GranuleFamily<false>>(s.H, nbt, false, a, hx, live, sync, st);
    if (rc == kNoInstantiation) { set_error("granule lstm: unsupported H=%d", s.H); return MDD_ERR_ARG; }
    return rc;
}

int init_granule_attributes() {
    if (int rc = init_persistent_attributes<GranuleFamily<false>>()) return rc;
    return init_persistent_attributes<GranuleFamily<true>>();
}

// The persistent layer kernels are written for a grid of exactly kPersistGrid workgroups (2 directions x 16 batch
// groups x 8 team members), ALL resident at once, one per CU.  persistent_grid_fits() asks the runtime whether a device
// with n_cu compute units can hold that grid (>= 1 workgroup of the largest configuration per CU, and enough CUs); when it
// cannot, the library uses the per-step kernels instead of risking a grid that waits for workgroups that never start.
int persistent_grid_fits(int n_cu) {
    using F = GranuleFamily<false>;
    return persist_grid_fits(n_cu, (const void *)F::kernel<384, kTeam8MaxTiles, false>(), F::lds(384, kTeam8MaxTiles)) &&
           persist_grid_fits(n_cu, (const void *)F::kernel<256, kTeam8MaxTiles, false>(), F::lds(256, kTeam8MaxTiles));
}

}  // namespace mdd
