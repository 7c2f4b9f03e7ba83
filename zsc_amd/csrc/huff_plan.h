/*
 * huff_plan.h -- kernel 3: per-block Huffman planning, one wavefront per block.
 *
 * Restates _tr_flush_block's decision half (reference src/trees.c:874-934):
 * symbol statistics, build_tree x3 (:559-652) with zlib's exact heap order
 * (:377-414 -- ties between equal frequency, equal depth nodes are resolved by
 * heap mechanics, so the heap is simulated, not replaced by a sort), gen_bitlen's
 * overflow repair (:477-507), scan_tree/build_bl_tree (:658-806), and the
 * stored / static / dynamic choice (:902-934).
 *
 * The heap is replayed step for step by lane 0 out of LDS; what has no serial
 * dependence is done by the 64 lanes: the symbol histogram (LDS atomics), the
 * heap's initial contents (ballot + prefix count), the bit counts of the block
 * (wave reduction), gen_codes (:518-549, a ballot per code length) and the
 * bit-length tree's part of the header.
 *
 * A heap entry is one 32-bit word, HP_WORD(freq, depth, node): smaller() (:377) is
 * one unsigned compare of two words' keys (word >> 10), and a level of pqdownheap
 * is one load of two neighbouring words.  An internal node's frequency lives only
 * in its word.  An entry that leaves the heap for the sorted list above heap_top
 * keeps its node number and swaps its key, dead from then on, for the number of
 * its parent (known at that moment), so that there is no parent[] array and
 * gen_bitlen's walk over the list is one dependent load per node.
 *
 * The key's fields: a block has at most 2^15 - 1 symbols (lit_bufsize - 1 at
 * mem_level 9) plus END_BLOCK, and forcing adds at most 2, so every frequency and
 * every sum is below 2^17.  A node of depth d in a tree built by merging the two
 * lightest nodes weighs at least Fib(d + 2) (1, 2, 3, 5, ...: the lighter child of
 * a merge is at least as heavy as the node merged before it), so with a total
 * below 2^17 no depth exceeds 24: five bits.  The lane emulation asserts both.
 *
 * 4.4 KiB of LDS per wave: 32 blocks are in flight per CU, the most it takes.
 * Output: code tables ready for the bit packer, the exact size of the block in
 * bits (opt_len/static_len are exact), and the dynamic block's header bits.
 */
#ifndef ZSC_HUFF_PLAN_H
#define ZSC_HUFF_PLAN_H

#include "wave.h"
#include "zsc_dev.h"
#ifdef ZSC_WAVE_EMU
#include <assert.h>
#define HP_ASSERT(x) assert(x)
#else
#define HP_ASSERT(x) ((void)0)
#endif

/* a hook for the lane emulation's tests: which rare paths a block took (0: a forced node, 1 + kind: the
 * overflow repair of that tree, 4 + type: the block's type) */
#ifndef HP_PATH
#define HP_PATH(id) ((void)0)
#endif

#define HP_LCODES 286
#define HP_DCODES 30
#define HP_BLCODES 19
#define HP_HEAP (2 * HP_LCODES + 1)

#define HP_NODE_MASK 1023u
#define HP_WORD(freq, depth, node) (((uint32_t)(freq) << 15) | ((uint32_t)(depth) << 10) | (uint32_t)(node))
#define HP_KEY(w) ((w) >> 10)
#define HP_FREQ(w) ((w) >> 15)
#define HP_DEPTH(w) (((w) >> 10) & 31u)
#define HP_NO_SYM 0xffffffffu /* (no symbol has a distance of 65 535) */
#ifndef HP_HIST_LOADS
#define HP_HIST_LOADS 4 /* symbols a lane asks for before it counts the first of them */
#endif

typedef struct {
    uint32_t heap[HP_HEAP + 1]; /* [1 .. heap_n] the heap, [heap_top .. HP_HEAP) the sorted list; the pair
                                   (heap[j], heap[j + 1]) of an even j is 8-byte aligned */
    uint32_t lfreq[HP_LCODES];  /* leaves only */
    uint32_t dfreq[HP_DCODES];
    uint32_t bfreq[HP_BLCODES];
    uint32_t bsend[HP_BLCODES]; /* the bit-length tree's codes as send_tree wants them: code | len << 16 */
    uint32_t per_len[16];       /* bl_count, only where the overflow repair needs it */
    /* code lengths: of every node while gen_bitlen runs, of the leaves from then on (each a multiple of four
     * bytes long: scan_tree and send_tree read them a word at a time, up to three bytes past max_code + 1) */
    uint8_t llen[HP_HEAP + 3];
    uint8_t dlen[2 * HP_DCODES + 4];
    uint8_t blen[2 * HP_BLCODES + 2];
} HpLds;

/* one of the three trees plus its static description (reference static_tree_desc, src/trees.c:237-252) */
template <int KIND> struct HpTree; /* 0 lit/len, 1 dist, 2 bit-length */
template <> struct HpTree<0> {
    enum { elems = HP_LCODES, max_len = 15, has_static = 1 };
};
template <> struct HpTree<1> {
    enum { elems = HP_DCODES, max_len = 15, has_static = 1 };
};
template <> struct HpTree<2> {
    enum { elems = HP_BLCODES, max_len = 7, has_static = 0 };
};

DEV uint32_t *hp_freq(HpLds *h, int kind)
{
    return kind == 0 ? h->lfreq : kind == 1 ? h->dfreq : h->bfreq;
}

DEV uint8_t *hp_len(HpLds *h, int kind)
{
    return kind == 0 ? h->llen : kind == 1 ? h->dlen : h->blen;
}

/* extra bits: reference src/trees.c:87-94, as arithmetic */
DEV int hp_extra(int kind, int sym)
{
    if (kind == 0) {
        if (sym < 265 || sym == 285)
            return 0;
        return (sym - 261) >> 2;
    }
    if (kind == 1)
        return sym < 4 ? 0 : (sym >> 1) - 1;
    return sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0;
}

DEV uint32_t hp_static_llen(uint32_t c) /* reference src/trees.c:110-169 */
{
    return c < 144 ? 8u : c < 256 ? 9u : c < 280 ? 7u : 8u;
}

/* length code of len-3 and distance code of dist-1: reference src/trees.c:180-223 */
DEV uint32_t hp_len_code(uint32_t lc)
{
    if (lc < 8)
        return lc;
    if (lc == 255)
        return 28;
    uint32_t e = 29u - (uint32_t)__builtin_clz(lc); /* floor(log2 lc) - 2 */
    return 4u * e + 4u + ((lc >> e) & 3u);
}

DEV uint32_t hp_dist_code(uint32_t d)
{
    if (d < 4)
        return d;
    uint32_t e = 30u - (uint32_t)__builtin_clz(d); /* floor(log2 d) - 1 */
    return 2u * e + 2u + ((d >> e) & 1u);
}

DEV uint32_t hp_len_base(uint32_t c) /* base_length, reference src/trees.c:225-228 */
{
    if (c < 8)
        return c;
    if (c == 28)
        return 0;
    uint32_t e = (c - 4) >> 2;
    return (4u + ((c - 4) & 3u)) << e;
}

DEV uint32_t hp_dist_base(uint32_t c) /* base_dist, reference src/trees.c:230-234 */
{
    if (c < 4)
        return c;
    uint32_t e = (c >> 1) - 1;
    return (2u + (c & 1u)) << e;
}

DEV uint32_t hp_bitrev(uint32_t v, int bits) /* bi_reverse, reference src/trees.c:1046-1058 */
{
    uint32_t r = 0;
    while (bits-- > 0) {
        r = (r << 1) | (v & 1u);
        v >>= 1;
    }
    return r;
}

/* pqdownheap, reference src/trees.c:387-414: `v` goes down from place k of a heap of n words */
DEV void hp_sift(uint32_t *heap, int n, int k, uint32_t v)
{
    for (int j = k << 1; j <= n; j <<= 1) {
        uint32_t c = heap[j];
        const uint32_t c1 = heap[j + 1]; /* (one load with heap[j]; past the heap's end where j == n, and unused) */
        if (j < n && HP_KEY(c1) <= HP_KEY(c)) {
            c = c1;
            j++;
        }
        if (HP_KEY(v) <= HP_KEY(c))
            break;
        heap[k] = c;
        k = j;
    }
    heap[k] = v;
}

/* build_tree's heap and gen_bitlen, reference src/trees.c:445-508 and :612-645: serial, lane 0 only.
 * `n` words are in the heap, `top` is max_code.  Leaves every node's length in len[]. */
template <int KIND>
DEV void hp_heap_and_lengths(HpLds *h, int n, int top)
{
    typedef HpTree<KIND> T;
    uint32_t *heap = h->heap;
    uint8_t *len = hp_len(h, KIND);
    for (int k = n / 2; k >= 1; k--)
        hp_sift(heap, n, k, heap[k]);

    int node = T::elems, ht = HP_HEAP;
    do { /* :624-640 */
        const uint32_t a = heap[1];
        const uint32_t last = heap[n];
        n--;
        hp_sift(heap, n, 1, last);
        const uint32_t b = heap[1];
        heap[--ht] = ((uint32_t)node << 10) | (a & HP_NODE_MASK);
        heap[--ht] = ((uint32_t)node << 10) | (b & HP_NODE_MASK);
        const uint32_t da = HP_DEPTH(a), db = HP_DEPTH(b);
        const uint32_t depth = (da >= db ? da : db) + 1u, freq = HP_FREQ(a) + HP_FREQ(b);
        HP_ASSERT(depth < 32u && freq < (1u << 17));
        hp_sift(heap, n, 1, HP_WORD(freq, depth, node));
        node++;
    } while (n >= 2);
    const int root = (int)(heap[1] & HP_NODE_MASK);

    /* gen_bitlen, :445-472 (the counts of the block's bits are taken from the final lengths, by all lanes) */
    int over = 0;
    len[root] = 0;
    uint32_t w = heap[ht];
    for (int i = ht; i < HP_HEAP; i++) {
        const uint32_t wn = heap[i + 1]; /* (asked for one node ahead; heap[HP_HEAP] is there and unused) */
        int bits = len[w >> 10] + 1;
        if (bits > (int)T::max_len) {
            bits = T::max_len;
            over++; /* internal nodes count too: :457 runs before :461 */
        }
        len[w & HP_NODE_MASK] = (uint8_t)bits;
        w = wn;
    }
    if (over > 0) {
        HP_PATH(1 + KIND);
        uint32_t *per_len = h->per_len;
        for (int b = 0; b < 16; b++)
            per_len[b] = 0;
        for (int i = ht; i < HP_HEAP; i++) {
            const int m = (int)(heap[i] & HP_NODE_MASK);
            if (m <= top)
                per_len[len[m]]++;
        }
        do { /* :477-489 */
            int bits = T::max_len - 1;
            while (per_len[bits] == 0)
                bits--;
            per_len[bits]--;
            per_len[bits + 1] += 2;
            per_len[T::max_len]--;
            over -= 2;
        } while (over > 0);
        int i = HP_HEAP;
        for (int bits = T::max_len; bits != 0; bits--) { /* :496-507 */
            uint32_t k = per_len[bits];
            while (k != 0) {
                const int m = (int)(heap[--i] & HP_NODE_MASK);
                if (m > top)
                    continue;
                len[m] = (uint8_t)bits;
                k--;
            }
        }
    }
}

/* build_tree + gen_bitlen + gen_codes of one tree, reference src/trees.c:426-652; called by the whole wave.
 * Adds the tree's part to opt_bits / static_bits (wave-uniform) and returns max_code.  The lit/len and distance
 * trees' codes go straight to the plan, the bit-length tree's to h->bsend. */
template <int KIND>
DEV int hp_build(HpLds *h, ZdBlockPlan *plan, uint32_t &opt_bits, uint32_t &static_bits)
{
    typedef HpTree<KIND> T;
    enum { NCH = (T::elems + WAVE - 1) / WAVE };
    uint32_t *const freq = hp_freq(h, KIND);
    uint8_t *const len = hp_len(h, KIND);
    int top = -1, n = 0;
    /* the symbols in use, in rising order, are the heap's first contents (:583-590) */
    for (int c = 0; c < NCH; c++) {
        LANEVAR(uint32_t, f);
        FOR_LANES
        {
            const int s = c * WAVE + LANE;
            LV(f) = s < (int)T::elems ? freq[s] : 0u;
            if (s < (int)T::elems)
                len[s] = 0;
        }
        const uint64_t m = BALLOT(f);
        FOR_LANES
        {
            if (LV(f))
                h->heap[n + 1 + POPC64(m & ((1ull << LANE) - 1ull))] = HP_WORD(LV(f), 0, c * WAVE + LANE);
        }
        if (m) {
            n += POPC64(m);
            top = c * WAVE + 63 - CLZ64(m);
        }
    }
    while (n < 2) { /* :595-610 */
        HP_PATH(0);
        const int node = top < 2 ? ++top : 0;
        n++;
        ON_LANE0
        {
            h->heap[n] = HP_WORD(1, 0, node);
            freq[node] = 1;
        }
        opt_bits--;
        if (T::has_static)
            static_bits -= KIND == 1 ? 5u : hp_static_llen((uint32_t)node);
    }
    WAVE_SYNC();
    ON_LANE0
    {
        hp_heap_and_lengths<KIND>(h, n, top);
    }
    WAVE_SYNC();

    /* the block's bits under this tree and under the static one (:461-471 and :501-505, summed up from the
     * final lengths: the low word counts the dynamic bits, the high word the static ones, each far below 2^32) */
    LANEARR(uint32_t, ln, NCH);
    LANEARR(uint32_t, cd, NCH);
    LANEVAR(uint64_t, bits);
    FOR_LANES
    {
        LV(bits) = 0;
    }
    UNROLL_FULL
    for (int c = 0; c < NCH; c++) {
        FOR_LANES
        {
            const int s = c * WAVE + LANE;
            uint32_t l = 0;
            if (s < (int)T::elems) {
                l = len[s];
                const uint32_t fr = freq[s], xb = (uint32_t)hp_extra(KIND, s);
                LV(bits) += (uint64_t)(fr * (l + xb));
                if (T::has_static)
                    LV(bits) += (uint64_t)(fr * ((KIND == 1 ? 5u : hp_static_llen((uint32_t)s)) + xb)) << 32;
            }
            LVA(ln, c) = l;
            LVA(cd, c) = 0;
        }
    }
    const uint64_t total = WAVE_SUM(bits);
    opt_bits += (uint32_t)total;
    static_bits += (uint32_t)(total >> 32);

    /* gen_codes, :518-549: the symbols of one length get consecutive codes in rising order, so a symbol's code
     * is its length's first one plus the number of lower symbols of that length */
    uint32_t code = 0, count = 0;
    for (int l = 1; l <= (int)T::max_len; l++) {
        code = (code + count) << 1;
        uint32_t run = code;
        UNROLL_FULL
        for (int c = 0; c < NCH; c++) {
            LANEVAR(uint32_t, is);
            FOR_LANES
            {
                LV(is) = LVA(ln, c) == (uint32_t)l;
            }
            const uint64_t m = BALLOT(is);
            FOR_LANES
            {
                if (LV(is))
                    LVA(cd, c) = run + (uint32_t)POPC64(m & ((1ull << LANE) - 1ull));
            }
            run += (uint32_t)POPC64(m);
        }
        count = run - code;
    }
    UNROLL_FULL
    for (int c = 0; c < NCH; c++) {
        FOR_LANES
        {
            const int s = c * WAVE + LANE;
            if (s < (int)T::elems) {
                const uint32_t l = LVA(ln, c);
                const uint32_t rev = l ? BREV32(LVA(cd, c)) >> (32u - l) : 0u; /* bi_reverse */
                if (KIND == 0) {
                    plan->lcode[s] = (uint16_t)rev;
                    plan->llen[s] = (uint8_t)l;
                } else if (KIND == 1) {
                    plan->dcode[s] = (uint16_t)rev;
                    plan->dlen[s] = (uint8_t)l;
                } else {
                    h->bsend[s] = rev | (l << 16);
                }
            }
        }
    }
    return top;
}

/* the code length of symbol i, through a word that holds four of them */
DEV uint32_t hp_len_at(const uint8_t *len, uint32_t &word, int i)
{
    if ((i & 3) == 0)
        __builtin_memcpy(&word, __builtin_assume_aligned(len + i, 4), 4);
    return (word >> ((i & 3) * 8)) & 0xffu;
}

/* scan_tree, reference src/trees.c:658-707 */
DEV void hp_scan(HpLds *h, uint8_t *len, int max_code)
{
    len[max_code + 1] = 0xff; /* guard, :674 */
    uint32_t word = 0;
    int prev = -1, next = (int)hp_len_at(len, word, 0), count = 0, hi = 7, lo = 4;
    if (next == 0) {
        hi = 138;
        lo = 3;
    }
    for (int n = 0; n <= max_code; n++) {
        int cur = next;
        next = (int)hp_len_at(len, word, n + 1);
        if (++count < hi && cur == next)
            continue;
        if (count < lo)
            LDS_ADD_U32(&h->bfreq[cur], (uint32_t)count);
        else if (cur != 0) {
            if (cur != prev)
                LDS_ADD_U32(&h->bfreq[cur], 1u);
            LDS_ADD_U32(&h->bfreq[16], 1u);
        } else if (count <= 10)
            LDS_ADD_U32(&h->bfreq[17], 1u);
        else
            LDS_ADD_U32(&h->bfreq[18], 1u);
        count = 0;
        prev = cur;
        if (next == 0) {
            hi = 138;
            lo = 3;
        } else if (cur == next) {
            hi = 6;
            lo = 3;
        } else {
            hi = 7;
            lo = 4;
        }
    }
}

/* header bit writer (send_bits into the plan's copy of the block header): the bits gather in a register
 * pair and leave as whole 32-bit words */
typedef struct {
    uint64_t acc;
    uint32_t fill, pos; /* bits in acc (below 32 between calls), bytes stored */
    uint8_t *out;       /* 4-byte aligned */
} HpBits;

DEV void hp_put(HpBits &w, uint32_t value, int nbits) /* nbits <= 32 */
{
    w.acc |= (uint64_t)value << w.fill;
    w.fill += (uint32_t)nbits;
    if (w.fill >= 32) {
        const uint32_t lo = (uint32_t)w.acc;
        __builtin_memcpy(__builtin_assume_aligned(w.out + w.pos, 4), &lo, 4);
        w.pos += 4;
        w.acc >>= 32;
        w.fill -= 32;
    }
}

/* send_tree, reference src/trees.c:713-773 (len[max_code + 1] still holds scan_tree's guard) */
DEV void hp_send_lengths(HpLds *h, HpBits &w, const uint8_t *len, int max_code)
{
    uint32_t word = 0;
    int prev = -1, next = (int)hp_len_at(len, word, 0), count = 0, hi = 7, lo = 4;
    if (next == 0) {
        hi = 138;
        lo = 3;
    }
    for (int n = 0; n <= max_code; n++) {
        int cur = next;
        next = (int)hp_len_at(len, word, n + 1);
        if (++count < hi && cur == next)
            continue;
        if (count < lo) {
            const uint32_t s = h->bsend[cur];
            do
                hp_put(w, s & 0xffffu, (int)(s >> 16));
            while (--count != 0);
        } else if (cur != 0) {
            if (cur != prev) {
                const uint32_t s = h->bsend[cur];
                hp_put(w, s & 0xffffu, (int)(s >> 16));
                count--;
            }
            const uint32_t s = h->bsend[16];
            hp_put(w, (s & 0xffffu) | ((uint32_t)(count - 3) << (s >> 16)), (int)(s >> 16) + 2);
        } else if (count <= 10) {
            const uint32_t s = h->bsend[17];
            hp_put(w, (s & 0xffffu) | ((uint32_t)(count - 3) << (s >> 16)), (int)(s >> 16) + 3);
        } else {
            const uint32_t s = h->bsend[18];
            hp_put(w, (s & 0xffffu) | ((uint32_t)(count - 11) << (s >> 16)), (int)(s >> 16) + 7);
        }
        count = 0;
        prev = cur;
        if (next == 0) {
            hi = 138;
            lo = 3;
        } else if (cur == next) {
            hi = 6;
            lo = 3;
        } else {
            hi = 7;
            lo = 4;
        }
    }
}

/* bl_order, reference src/trees.c:96-99: five bits a symbol, twelve symbols in the first word */
DEV uint32_t hp_bl_order(int r)
{
    const uint64_t a = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 |
                       6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
    const uint64_t b = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    return (uint32_t)((r < 12 ? a >> (5 * r) : b >> (5 * (r - 12))) & 31u);
}

/* plan one block: `syms` points at the block's first symbol */
DEV void huff_plan_block(const uint32_t *syms, const ZdBlockRec *rec, uint32_t strategy,
                         ZdBlockPlan *plan, HpLds *h)
{
    const uint32_t count = rec->sym_count;
    /* init_block, reference src/trees.c:336-356 */
    for (int i = 0; i < HP_LCODES; i += WAVE) {
        FOR_LANES
        {
            if (i + LANE < HP_LCODES)
                h->lfreq[i + LANE] = i + LANE == 256 ? 1u : 0u; /* (END_BLOCK) */
        }
    }
    for (int i = 0; i < HP_DCODES; i += WAVE) {
        FOR_LANES
        {
            if (i + LANE < HP_DCODES)
                h->dfreq[i + LANE] = 0;
            if (i + LANE < HP_BLCODES)
                h->bfreq[i + LANE] = 0;
        }
    }
    WAVE_SYNC();
    /* symbol statistics, reference include/zsc/deflate.h:338-354; HP_HIST_LOADS loads in flight per lane */
    for (uint32_t s = 0; s < count; s += HP_HIST_LOADS * WAVE) {
        FOR_LANES
        {
            uint32_t v[HP_HIST_LOADS];
            UNROLL_FULL
            for (int k = 0; k < HP_HIST_LOADS; k++) {
                const uint32_t i = s + (uint32_t)(k * WAVE + LANE);
                v[k] = i < count ? syms[i] : HP_NO_SYM;
            }
            UNROLL_FULL
            for (int k = 0; k < HP_HIST_LOADS; k++) {
                const uint32_t dist = v[k] >> 16, lc = v[k] & 0xff;
                if (v[k] == HP_NO_SYM) {
                } else if (dist == 0) {
                    LDS_ADD_U32(&h->lfreq[lc], 1u);
                } else {
                    LDS_ADD_U32(&h->lfreq[257 + hp_len_code(lc)], 1u);
                    LDS_ADD_U32(&h->dfreq[hp_dist_code(dist - 1)], 1u);
                }
            }
        }
    }
    WAVE_SYNC();
    uint32_t opt_bits = 0, static_bits = 0;
    const int lmax = hp_build<0>(h, plan, opt_bits, static_bits);
    const int dmax = hp_build<1>(h, plan, opt_bits, static_bits);
    /* build_bl_tree, reference src/trees.c:779-806 */
    ON_LANE0
    {
        hp_scan(h, h->llen, lmax);
        hp_scan(h, h->dlen, dmax);
    }
    WAVE_SYNC();
    hp_build<2>(h, plan, opt_bits, static_bits);
    WAVE_SYNC();
    /* the last bit-length code in use in bl_order, and the lengths up to it, three bits each */
    int last_bl = 0;
    uint64_t bl_bits = 0;
    for (int i = 0; i < HP_BLCODES; i += WAVE) {
        LANEVAR(uint32_t, bl);
        FOR_LANES
        {
            LV(bl) = i + LANE < HP_BLCODES ? h->bsend[hp_bl_order(i + LANE)] >> 16 : 0u;
        }
        const uint64_t m = BALLOT(bl);
        if (m)
            last_bl = i + 63 - CLZ64(m);
        LANEVAR(uint64_t, part);
        FOR_LANES
        {
            LV(part) = i + LANE < HP_BLCODES ? (uint64_t)LV(bl) << (3 * (i + LANE)) : 0ull;
        }
        bl_bits += WAVE_SUM(part);
    }
    if (last_bl < 3)
        last_bl = 3;
    opt_bits += 3u * ((uint32_t)last_bl + 1u) + 5u + 5u + 4u;

    /* reference src/trees.c:902-934 */
    uint32_t opt_bytes = (opt_bits + 3 + 7) >> 3;
    const uint32_t static_bytes = (static_bits + 3 + 7) >> 3;
    if (static_bytes <= opt_bytes)
        opt_bytes = static_bytes;
    uint32_t type;
    if (rec->in_len + 4 <= opt_bytes && rec->stored_ok)
        type = ZD_BT_STORED;
    else if (strategy == 4 || static_bytes == opt_bytes)
        type = ZD_BT_STATIC;
    else
        type = ZD_BT_DYNAMIC;
    ON_LANE0
    {
        HP_PATH(4 + type);
        HpBits w = {0, 0, 0, plan->hdr};
        if (type == ZD_BT_DYNAMIC) {
            /* send_all_trees, reference src/trees.c:813-833 */
            hp_put(w, (uint32_t)(lmax + 1 - 257) | (uint32_t)(dmax + 1 - 1) << 5 | (uint32_t)(last_bl + 1 - 4) << 10, 14);
            const int nb = 3 * (last_bl + 1);
            const uint64_t sent = nb < 64 ? bl_bits & ((1ull << nb) - 1ull) : bl_bits;
            hp_put(w, (uint32_t)sent, nb < 32 ? nb : 32);
            if (nb > 32)
                hp_put(w, (uint32_t)(sent >> 32), nb - 32);
            hp_send_lengths(h, w, h->llen, lmax);
            hp_send_lengths(h, w, h->dlen, dmax);
        }
        plan->type = type;
        plan->hdr_bits = w.pos * 8 + w.fill;
        if (w.fill) {
            const uint32_t lo = (uint32_t)w.acc;
            __builtin_memcpy(__builtin_assume_aligned(w.out + w.pos, 4), &lo, 4);
        }
        plan->body_bits = type == ZD_BT_DYNAMIC ? 3u + opt_bits : type == ZD_BT_STATIC ? 3u + static_bits : 0u;
        plan->bit_off = 0;
    }
    WAVE_SYNC(); /* (the next block of this wave's slot reuses the LDS image) */
}

#endif
