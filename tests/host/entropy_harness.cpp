// Host harness (tests only): exposes the serial table-construction functions of
// vbz_compression_amd/csrc/zstd_entropy.h to ctypes so the CPU suite can check them against
// what libzstd emits for the same histogram, the table readers of zstd_tables.h to check them
// against the oracle's restatement, and the header readers of zstd_frame.h.  Built by tests/entropy_host.py with g++.
#include <cstring>
#include "zstd_entropy.h"
#include "zstd_tables.h"
#include "zstd_frame.h"
#include "zstd_reference_huffman.h"   // libzstd's construction: the yardstick (BSD notice inside)

using namespace vbzhip;

extern "C" {

int h_huf_build(const uint32_t* count, uint32_t maxSymbolValue, uint32_t maxNbBits, uint8_t* nbBits, uint16_t* code)
{
    static HufBuildWksp w;
    return (int)huf_build(count, maxSymbolValue, maxNbBits, nbBits, code, &w);
}

int h_huf_build_pm(const uint32_t* count, uint32_t maxSymbolValue, uint32_t maxNbBits, uint8_t* nbBits, uint16_t* code)
{
    static HufPmWksp w;
    return (int)huf_build_pm(count, maxSymbolValue, maxNbBits, nbBits, code, &w);
}

uint32_t h_optimal_table_log(uint32_t maxTableLog, uint32_t srcSize, uint32_t maxSymbolValue, uint32_t minus)
{
    return optimal_table_log(maxTableLog, srcSize, maxSymbolValue, minus);
}

// zstd_tables.h with plain arrays for the policies
struct HostFse
{
    int16_t nrm[256];
    uint16_t nx[256];
    uint32_t tab[512];
    int norm(int s) const { return nrm[s]; }
    void set_norm(int s, int c) { nrm[s] = (int16_t)c; }
    uint16_t& next(int s) { return nx[s]; }
    uint32_t& cell(int u) { return tab[u]; }
    void entry(int u, uint32_t s, uint32_t nb, uint32_t base) { tab[u] = fse_entry(s, nb, base); }
};

int h_fse_read_ncount(const uint8_t* p, int n, int max_symbol, int max_log, int16_t* norm, int* log, int* nsym)
{
    return fse_read_ncount([&](uint32_t pos, int k) { return le_bits(p, n, pos, k); }, n, max_symbol, max_log,
                           [&](int s, int c) { norm[s] = (int16_t)c; }, log, nsym);
}

// cells[u] = symbol | nbBits << 8 | base << 16
int h_fse_build(const int16_t* norm, int nsym, int log, uint32_t* cells)
{
    static HostFse t;
    memcpy(t.nrm, norm, sizeof(int16_t) * (size_t)nsym);
    if (!fse_build(t, nsym, log)) return -1;
    memcpy(cells, t.tab, sizeof(uint32_t) << log);
    return 0;
}

// weights[0 .. *nw) of a tree description; returns bytes used, -1 or -2 (a table log beyond max_log)
int h_huf_read_weights(const uint8_t* p, int n, int max_log, uint8_t* weights, int* nw, int* log)
{
    struct Src
    {
        const uint8_t* p;
        int hb;
        uint32_t byte(int i) const { return p[i]; }
        uint32_t bits(uint32_t pos, int k) const { return le_bits(p + 1, hb, pos, k); }
    } src = { p, n > 0 ? p[0] : 0 };
    static HostFse t;
    return huf_read_weights(src, n, max_log, t, [&](int i, uint32_t w) { weights[i] = (uint8_t)w; }, nw, log);
}

// zstd_frame.h over plain byte arrays.  h_frame_header: 1 if the header ends inside the n bytes; out[] = { magic, fhd, len, wlog,
// did_bytes, did, fcs_bytes, checksum }, big[] = { fcs, window }
int h_frame_header(const uint8_t* p, uint32_t n, uint32_t* out, uint64_t* big)
{
    ZFrameHeader h;
    const bool whole = zstd_frame_header([&](uint32_t i) { return (uint32_t)p[i]; }, n, &h);
    const uint32_t o[8] = { h.magic, h.fhd, h.len, h.wlog, h.did_bytes, h.did, h.fcs_bytes, h.checksum };
    memcpy(out, o, sizeof(o));
    big[0] = h.fcs;
    big[1] = h.window;
    return whole ? 1 : 0;
}

// out[] = { last, type, size, src }
void h_block_header(uint32_t bh, uint32_t* out)
{
    const ZBlockHeader k = zstd_block_header(bh);
    out[0] = k.last;
    out[1] = k.type;
    out[2] = k.size;
    out[3] = k.src;
}

// out[] = { type, fmt, hsize, regen, csize, streams }
void h_lit_header(uint64_t v, uint32_t* out)
{
    const ZLitHeader l = zstd_lit_header(v);
    const uint32_t o[6] = { l.type, l.fmt, l.hsize, l.regen, l.csize, l.streams };
    memcpy(out, o, sizeof(o));
}

uint32_t h_nseq(const uint8_t* p, uint32_t n, uint32_t* used)
{
    return zstd_nseq([&](uint32_t i) { return (uint32_t)p[i]; }, n, used);
}

uint32_t h_huf_desc_size(uint32_t hb) { return huf_desc_size(hb); }

static uint32_t le32(const uint8_t* p, uint32_t o)
{
    uint32_t v;
    memcpy(&v, p + o, 4);
    return v;
}

// out[] = { off, count, spacing }
void h_checkpoints(const uint8_t* p, uint32_t n, uint32_t* out)
{
    const ZCheckpoints c = zstd_checkpoints([&](uint32_t o) { return le32(p, o); }, n);
    out[0] = c.off;
    out[1] = c.count;
    out[2] = c.spacing;
}

uint32_t h_skip_frames(const uint8_t* p, uint32_t pos, uint32_t n)
{
    return zstd_skip_frames([&](uint32_t o) { return le32(p, o); }, pos, n);
}

int h_huf_write_tree(uint8_t* dst, int cap, const uint8_t* nbBits, uint32_t maxSymbolValue, uint32_t huffLog)
{
    static FseWeightWksp w;
    uint8_t weights[260];
    return huf_write_tree(dst, cap, nbBits, maxSymbolValue, huffLog, weights, &w);
}

// Which way a weight list (weights[0 .. wtSize), the last symbol's left out as in a tree description) takes through huf_write_tree:
// out[] = { method, kind, low, size }.  method: 0 the weights are never normalised (fewer than two, all equal, or every value once:
// huf_compress_weights returns before fse_normalize), 1 / 2 fse_normalize's first / second method; kind: 0 FSE-coded, 1 direct 4-bit
// weights, 2 no description can be written; low: weight values at or below the low-probability threshold (norm = lowProbCount);
// size: the description's bytes (0 for kind 2).  The decision between the methods is restated here (fse_normalize does not report
// it) and held against fse_normalize's own result: -1 if the first method's restatement gives other counts than the function.
int h_weights_report(const uint8_t* weights, uint32_t wtSize, uint32_t* out)
{
    static FseWeightWksp w;
    uint8_t scratch[260], dst[300];
    out[0] = out[1] = out[2] = out[3] = 0;
    for (int i = 0; i < 16; ++i) w.count[i] = 0;
    for (uint32_t i = 0; i < wtSize; ++i) {
        if (weights[i] > HUF_ABS_MAX_BITS) return -1;
        w.count[weights[i]]++;
        scratch[i] = weights[i];
    }
    uint32_t maxSV = HUF_ABS_MAX_BITS, maxCount = 0;
    while (maxSV > 0 && w.count[maxSV] == 0) maxSV--;
    for (uint32_t s = 0; s <= maxSV; ++s) maxCount = w.count[s] > maxCount ? w.count[s] : maxCount;
    if (wtSize > 1 && maxCount != wtSize && maxCount != 1) {
        const uint32_t tableLog = optimal_table_log(6, wtSize, maxSV, 2), total = wtSize;
        const uint64_t scale = 62 - tableLog, step = ((uint64_t)1 << 62) / total, vStep = 1ull << (scale - 20);
        const uint32_t rtb[8] = { 0, 473195, 504333, 520860, 550000, 700000, 750000, 830000 };
        int still = 1 << tableLog, first[16];
        uint32_t largest = 0;
        int largestP = 0;
        for (uint32_t s = 0; s <= maxSV; ++s) {
            first[s] = 0;
            if (w.count[s] == 0) continue;
            if (w.count[s] <= (total >> tableLog)) { first[s] = 1; still--; out[2]++; continue; }
            int proba = (int)((w.count[s] * step) >> scale);
            if (proba < 8 && ((w.count[s] * step) - ((uint64_t)proba << scale)) > vStep * rtb[proba]) proba++;
            if (proba > largestP) { largestP = proba; largest = s; }
            first[s] = proba;
            still -= proba;
        }
        out[0] = -still >= (first[largest] >> 1) ? 2 : 1;
        int16_t norm[16];
        if (fse_normalize(norm, tableLog, w.count, total, maxSV, 1) <= 0) return -1;
        if (out[0] == 1) {
            first[largest] += still;
            for (uint32_t s = 0; s <= maxSV; ++s)
                if (norm[s] != first[s]) return -1;
        }
    }
    const int ts = huf_write_tree(dst, 300, nullptr, wtSize, 0, scratch, &w, true);
    out[1] = ts < 0 ? 2u : (dst[0] >= 128 ? 1u : 0u);
    out[3] = ts < 0 ? 0u : (uint32_t)ts;
    return 0;
}
}

// ---- prototype of the "zero-run sequences" block (tests only): the serial statement of what the device
// encoder emits for the control-byte region.  One compressed block: raw literals + sequences whose
// matches are all offset-1 runs (repeat offset 1 of a fresh frame), LL/ML predefined, OF RLE(code 0).
extern "C" int h_encode_zero_run_frame(const uint8_t* k, uint32_t K, uint8_t* out, uint32_t cap, uint32_t rmin)
{
    static SeqCTables T;
    seq_build_default_ctables(&T);
    // tokenise: literals = bytes not in the tail of a zero run of length >= rmin
    static uint8_t lit[1 << 17];
    static uint32_t LL[1 << 14], ML[1 << 14];
    uint32_t nlit = 0, nseq = 0, litsince = 0;
    for (uint32_t p = 0; p < K;) {
        if (k[p] == 0) {
            uint32_t e = p;
            while (e < K && k[e] == 0) ++e;
            if (e - p >= rmin) {
                lit[nlit++] = 0;
                ++litsince;
                LL[nseq] = litsince;
                ML[nseq] = e - p - 1;
                ++nseq;
                litsince = 0;
                p = e;
                continue;
            }
            for (; p < e; ++p) { lit[nlit++] = 0; ++litsince; }
            continue;
        }
        lit[nlit++] = k[p++];
        ++litsince;
    }
    if (nseq == 0 || K > (128u << 10)) return -1;
    uint8_t* op = out;
    // frame header
    const uint32_t magic = 0xFD2FB528u;
    memcpy(op, &magic, 4); op += 4;
    if (K < 256) { *op++ = 0x20; *op++ = (uint8_t)K; }
    else if (K < 65536 + 256) { *op++ = 0x60; uint16_t v = (uint16_t)(K - 256); memcpy(op, &v, 2); op += 2; }
    else { *op++ = 0xA0; memcpy(op, &K, 4); op += 4; }
    uint8_t* bh = op; op += 3;
    // raw literals header
    if (nlit < 32) *op++ = (uint8_t)(nlit << 3);
    else if (nlit < 4096) { *op++ = (uint8_t)((nlit << 4) | 4); *op++ = (uint8_t)(nlit >> 4); }
    else { *op++ = (uint8_t)((nlit << 4) | 12); *op++ = (uint8_t)(nlit >> 4); *op++ = (uint8_t)(nlit >> 12); }
    memcpy(op, lit, nlit); op += nlit;
    // sequences header
    if (nseq < 128) *op++ = (uint8_t)nseq;
    else if (nseq < 0x7F00) { *op++ = (uint8_t)((nseq >> 8) + 128); *op++ = (uint8_t)nseq; }
    else { *op++ = 255; uint16_t v = (uint16_t)(nseq - 0x7F00); memcpy(op, &v, 2); op += 2; }
    *op++ = 0x10;  // LL predefined, OF RLE, ML predefined
    *op++ = 0;     // OF code 0: repeat offset 1 (== 1 in a fresh frame)
    BitW bw; bw.acc = 0; bw.nbits = 0; bw.p = op; bw.end = out + cap;
    uint32_t stLL, stML, c, ex, nb;
    auto init2 = [&](uint32_t& st, const uint16_t* stab, const uint32_t* dnb, const int32_t* dfs, uint32_t sym) {
        uint32_t nbo = (dnb[sym] + (1u << 15)) >> 16;
        uint32_t v = (nbo << 16) - dnb[sym];
        st = stab[(int32_t)(v >> nbo) + dfs[sym]];
    };
    auto enc = [&](uint32_t& st, const uint16_t* stab, const uint32_t* dnb, const int32_t* dfs, uint32_t sym) {
        uint32_t nbo = (st + dnb[sym]) >> 16;
        bitw_add(bw, st, nbo);
        st = stab[(int32_t)(st >> nbo) + dfs[sym]];
    };
    {
        uint32_t lc, lex, lnb, mc, mex, mnb;
        seq_ll_code(LL[nseq - 1], &lc, &lex, &lnb);
        seq_ml_code(ML[nseq - 1], &mc, &mex, &mnb);
        init2(stML, T.ml_state, T.ml_dnb, T.ml_dfs, mc);
        init2(stLL, T.ll_state, T.ll_dnb, T.ll_dfs, lc);
        bitw_add(bw, lex, lnb); bitw_flush(bw);
        bitw_add(bw, mex, mnb); bitw_flush(bw);
    }
    for (int n = (int)nseq - 2; n >= 0; --n) {
        uint32_t lc, lex, lnb, mc, mex, mnb;
        seq_ll_code(LL[n], &lc, &lex, &lnb);
        seq_ml_code(ML[n], &mc, &mex, &mnb);
        enc(stML, T.ml_state, T.ml_dnb, T.ml_dfs, mc);
        enc(stLL, T.ll_state, T.ll_dnb, T.ll_dfs, lc);
        bitw_flush(bw);
        bitw_add(bw, lex, lnb); bitw_flush(bw);
        bitw_add(bw, mex, mnb); bitw_flush(bw);
    }
    (void)c; (void)ex; (void)nb;
    bitw_add(bw, stML, SEQ_DEF_LOG); bitw_flush(bw);
    bitw_add(bw, stLL, SEQ_DEF_LOG); bitw_flush(bw);
    bitw_add(bw, 1, 1); bitw_flush(bw);
    if (bw.nbits > 0) *bw.p++ = (uint8_t)bw.acc;
    op = bw.p;
    const uint32_t bsize = (uint32_t)(op - bh - 3);
    const uint32_t hv = (bsize << 3) | (2u << 1) | 1u;
    bh[0] = (uint8_t)hv; bh[1] = (uint8_t)(hv >> 8); bh[2] = (uint8_t)(hv >> 16);
    return (int)(op - out);
}
