/*
 * emu_dict.cpp -- TEST INFRASTRUCTURE ONLY: a stand-alone program that inflates streams with the decoder's
 * dictionary variant (zsc_amd/csrc/inflate.h, INF_SEC_DICT) on the lane emulation (wave.h,
 * -DZSC_WAVE_EMU), as the runtime runs it: the dictionary's id and window image made as k_dict_setup makes
 * them, then k_inflate_dict's decode with its relaunches after data errors.
 *
 * usage: emu_dict CASES OUT
 * CASES holds records of int32 window_bits, uint32 dest_cap, uint32 dict_len (0xFFFFFFFF: no dictionary),
 * uint32 n, the dictionary's bytes and the n bytes of the stream.  One line per record: status out_len
 * consumed clean -- clean is 1 when every byte of the destination beyond out_len (64 guard bytes behind
 * dest_cap included) is untouched.  The out_len bytes of every record are appended to OUT.
 *
 * The image is allocated at the dictionary's own size, so that under AddressSanitizer a read before the
 * dictionary's first byte is a read outside the allocation.
 */
#define ZSC_WAVE_EMU 1
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "../../zsc_amd/csrc/inflate.h"

#define NO_DICT 0xffffffffu
#define GUARD 64u
#define FILL 0xA5

static int dict_one(const uint8_t *src, uint32_t n, int window_bits, uint32_t cap, const uint8_t *dict,
                    uint32_t dict_len, std::vector<uint8_t> &out, uint32_t *consumed, int *clean)
{
    std::vector<uint8_t> in((size_t)n + 64, 0);
    if (n)
        memcpy(in.data(), src, n);
    InfDict dc = {nullptr, 0u, 0u};
    uint8_t *img = nullptr;
    if (dict_len != NO_DICT) {
        const uint32_t have = std::min(dict_len, INF_WIN);
        img = (uint8_t *)malloc(have ? have : 1u);
        if (have)
            memcpy(img, dict + (dict_len - have), have);
        dc.win = (const uint8_t *)((uintptr_t)img + have - INF_WIN); /* win[INF_WIN - d]: the byte d before the start */
        dc.len = dict_len;
        dc.id = ck_adler32(dict, dict_len);
    }
    uint8_t *dst = (uint8_t *)malloc((size_t)cap + GUARD);
    memset(dst, FILL, (size_t)cap + GUARD);
    InfLds *lds = (InfLds *)malloc(sizeof(InfLds));
    memset(lds, 0x3C, sizeof(InfLds));
    static uint32_t crc_table[1][256];
    lds->cktab = crc_table;
    InfResult res;
    memset(&res, 0, sizeof res);
    InfJob job = {in.data(), n, dst, cap, window_bits};
    inflate_dict_with_resync(job, dc, lds, &res);
    *clean = res.out_len <= cap;
    for (size_t k = res.out_len; k < (size_t)cap + GUARD && *clean; k++)
        *clean = dst[k] == FILL;
    out.assign(dst, dst + std::min(res.out_len, cap));
    *consumed = res.consumed;
    free(lds);
    free(dst);
    free(img);
    return res.status;
}

int main(int argc, char **argv)
{
    if (argc != 3) {
        fprintf(stderr, "usage: %s CASES OUT\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    FILE *o = fopen(argv[2], "wb");
    if (!o) {
        perror(argv[2]);
        return 2;
    }
    for (;;) {
        uint32_t h[4];
        const size_t got = fread(h, 4, 4, f);
        if (got == 0)
            break;
        if (got != 4) {
            fprintf(stderr, "short record header\n");
            return 2;
        }
        const uint32_t dl = h[2] == NO_DICT ? 0u : h[2];
        std::vector<uint8_t> d((size_t)dl + 1), s((size_t)h[3] + 1);
        if ((dl && fread(d.data(), 1, dl, f) != dl) || (h[3] && fread(s.data(), 1, h[3], f) != h[3])) {
            fprintf(stderr, "short record\n");
            return 2;
        }
        std::vector<uint8_t> out;
        uint32_t consumed = 0;
        int clean = 0;
        const int rc = dict_one(s.data(), h[3], (int32_t)h[0], h[1], d.data(), h[2], out, &consumed, &clean);
        printf("%d %u %u %d\n", rc, (unsigned)out.size(), consumed, clean);
        if (!out.empty() && fwrite(out.data(), 1, out.size(), o) != out.size()) {
            perror(argv[2]);
            return 2;
        }
    }
    fclose(o);
    fclose(f);
    return 0;
}
