// Host side of the JPEG decoder: marker parsing and Huffman decoding of a baseline file into quantised
// coefficients.  Plain C++17: no HIP call, no global state, no allocation - two threads may decode at once.  Included by
// jpeg_decode.hip (which exports the two functions) and by tools/jpeg_host_check.cpp (a stand-alone program for sanitizer runs).
//
// Every read of the file goes through an explicit bound against n, every write through one against the caller's element count: no
// input makes either function touch memory outside [data, data + n), info[SPE_JPEG_INFO_INTS] and coef[coef_elems].
#ifndef SPE_JPEG_ENTROPY_H
#define SPE_JPEG_ENTROPY_H
#include <stdint.h>
#include <string.h>

#define SPE_JPEG_UNSUPPORTED (-7)       // a valid file of a form this decoder does not take
#define SPE_JPEG_CORRUPT (-8)           // not a decodable file
#define SPE_JPEG_INFO_INTS 224

// info[]: the frame as the device pass needs it.  Per-component triples are indexed by the component's position in the frame.
enum { JI_WIDTH, JI_HEIGHT, JI_NCOMP, JI_HMAX, JI_VMAX, JI_RESTART, JI_MCUX, JI_MCUY, JI_H /* 3 */, JI_V = 11 /* 3 */,
       JI_BW = 14 /* 3: blocks across, whole MCUs */, JI_BH = 17 /* 3 */, JI_NBLK = 20 /* 3 */, JI_BLOCKS = 23 /* all components */,
       JI_REASON = 24, JI_SCAN = 25 /* offset of the first entropy-coded byte */, JI_QT = 32 /* 3 x 64, natural order */ };

// why a file was refused (info[JI_REASON], *reason); spe_amd/jpeg.py has the texts
enum { JR_NONE, JR_PROGRESSIVE, JR_PROCESS, JR_PRECISION, JR_QT16, JR_NCOMP, JR_SAMPLING, JR_SCANS, JR_ADOBE, JR_RGB_IDS, JR_DNL,
       JR_TRUNCATED = 32, JR_MARKER, JR_LENGTH, JR_NO_TABLE, JR_BAD_CODE, JR_RUN, JR_RESTART, JR_HEADER, JR_BUFFER = 64 };

static const unsigned char spe_jpeg_natural[64] = {
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct spe_jpeg_rawhuff { unsigned char defined, counts[16], symbols[256]; };
struct spe_jpeg_header {
    int width, height, ncomp, restart;
    int id[3], h[3], v[3], tq[3], td[3], ta[3];
    unsigned char qt_defined[4], qt[4][64];          // natural order
    spe_jpeg_rawhuff huff[2][4];                     // [class][id]
    long scan;
};

#define JPG_FAIL(status, why) do { *reason = (why); return (status); } while (0)

// markers up to and including the scan header
static inline int spe_jpeg_parse(const unsigned char* d, long n, spe_jpeg_header* hd, int* reason) {
    memset(hd, 0, sizeof(*hd));
    *reason = JR_NONE;
    if (!d || n < 2) JPG_FAIL(SPE_JPEG_CORRUPT, JR_TRUNCATED);
    if (d[0] != 0xFF || d[1] != 0xD8) JPG_FAIL(SPE_JPEG_CORRUPT, JR_MARKER);
    long p = 2;
    bool frame = false, jfif = false, adobe = false;
    int transform = -1;
    for (;;) {
        if (p >= n) JPG_FAIL(SPE_JPEG_CORRUPT, JR_TRUNCATED);
        if (d[p] != 0xFF) JPG_FAIL(SPE_JPEG_CORRUPT, JR_MARKER);
        while (p < n && d[p] == 0xFF) ++p;                                   // fill bytes
        if (p >= n) JPG_FAIL(SPE_JPEG_CORRUPT, JR_TRUNCATED);
        const int m = d[p++];
        if (m == 0xC2) JPG_FAIL(SPE_JPEG_UNSUPPORTED, JR_PROGRESSIVE);
        if ((m >= 0xC1 && m <= 0xCF && m != 0xC4 && m != 0xC8)) JPG_FAIL(SPE_JPEG_UNSUPPORTED, JR_PROCESS);   // extended, lossless, arithmetic
        const bool known = m == 0xC0 || m == 0xC4 || m == 0xDA || m == 0xDB || m == 0xDD || (m >= 0xE0 && m <= 0xEF) || m == 0xFE;
        if (!known) JPG_FAIL(SPE_JPEG_CORRUPT, JR_MARKER);
        if (p + 2 > n) JPG_FAIL(SPE_JPEG_CORRUPT, JR_TRUNCATED);
        const long L = ((long)d[p] << 8) | d[p + 1];
        if (L < 2) JPG_FAIL(SPE_JPEG_CORRUPT, JR_LENGTH);
        if (p + L > n) JPG_FAIL(SPE_JPEG_CORRUPT, JR_TRUNCATED);
        const unsigned char* s = d + p + 2;
        long sl = L - 2;
        p += L;
        if (m == 0xDB) {
            while (sl > 0) {
                const int pq = s[0] >> 4, tq = s[0] & 15;
                if (tq > 3 || pq > 1) JPG_FAIL(SPE_JPEG_CORRUPT, JR_HEADER);
                if (pq == 1) JPG_FAIL(SPE_JPEG_UNSUPPORTED, JR_QT16);
                if (sl < 65) JPG_FAIL(SPE_JPEG_CORRUPT, JR_LENGTH);
                for (int k = 0; k < 64; ++k) hd->qt[tq][spe_jpeg_natural[k]] = s[1 + k];
                hd->qt_defined[tq] = 1;
                s += 65; sl -= 65;
            }
        } else if (m == 0xC4) {
            while (sl > 0) {
                if (sl < 17) JPG_FAIL(SPE_JPEG_CORRUPT, JR_LENGTH);
                const int tc = s[0] >> 4, th = s[0] & 15;
                if (tc > 1 || th > 3) JPG_FAIL(SPE_JPEG_CORRUPT, JR_HEADER);
                int total = 0;
                for (int k = 0; k < 16; ++k) total += s[1 + k];
                if (total > 256 || sl < 17 + total) JPG_FAIL(SPE_JPEG_CORRUPT, JR_LENGTH);
                spe_jpeg_rawhuff* t = &hd->huff[tc][th];
                memcpy(t->counts, s + 1, 16);
                memset(t->symbols, 0, 256);
                memcpy(t->symbols, s + 17, (size_t)total);
                t->defined = 1;
                s += 17 + total; sl -= 17 + total;
            }
        } else if (m == 0xC0) {
            if (frame) JPG_FAIL(SPE_JPEG_CORRUPT, JR_HEADER);
            if (sl < 6) JPG_FAIL(SPE_JPEG_CORRUPT, JR_LENGTH);
            const int prec = s[0], nf = s[5];
            hd->height = (s[1] << 8) | s[2];
            hd->width = (s[3] << 8) | s[4];
            if (prec == 12 || prec == 16) JPG_FAIL(SPE_JPEG_UNSUPPORTED, JR_PRECISION);
            if (prec != 8 || hd->width == 0 || nf == 0) JPG_FAIL(SPE_JPEG_CORRUPT, JR_HEADER);
            if (sl != 6 + 3 * (long)nf) JPG_FAIL(SPE_JPEG_CORRUPT, JR_LENGTH);
            if (nf != 1 && nf != 3) JPG_FAIL(SPE_JPEG_UNSUPPORTED, JR_NCOMP);
            if (hd->height == 0) JPG_FAIL(SPE_JPEG_UNSUPPORTED, JR_DNL);        // the height would come in a DNL segment after the scan
            hd->ncomp = nf;
            for (int c = 0; c < nf; ++c) {
                hd->id[c] = s[6 + 3 * c];
                hd->h[c] = s[7 + 3 * c] >> 4;
                hd->v[c] = s[7 + 3 * c] & 15;
                hd->tq[c] = s[8 + 3 * c];
                if (hd->h[c] < 1 || hd->h[c] > 4 || hd->v[c] < 1 || hd->v[c] > 4 || hd->tq[c] > 3) JPG_FAIL(SPE_JPEG_CORRUPT, JR_HEADER);
            }
            frame = true;
        } else if (m == 0xDD) {
            if (sl != 2) JPG_FAIL(SPE_JPEG_CORRUPT, JR_LENGTH);
            hd->restart = (s[0] << 8) | s[1];
        } else if (m == 0xE0) {
            if (sl >= 5 && memcmp(s, "JFIF", 5) == 0) jfif = true;
        } else if (m == 0xEE) {
            if (sl >= 12 && memcmp(s, "Adobe", 5) == 0) { adobe = true; transform = s[11]; }
        } else if (m == 0xDA) {
            if (!frame) JPG_FAIL(SPE_JPEG_CORRUPT, JR_HEADER);
            if (sl < 1) JPG_FAIL(SPE_JPEG_CORRUPT, JR_LENGTH);
            const int ns = s[0];
            if (ns < 1 || ns > 4) JPG_FAIL(SPE_JPEG_CORRUPT, JR_HEADER);
            if (sl != 4 + 2 * (long)ns) JPG_FAIL(SPE_JPEG_CORRUPT, JR_LENGTH);
            if (ns != hd->ncomp) JPG_FAIL(SPE_JPEG_UNSUPPORTED, JR_SCANS);
            for (int c = 0; c < ns; ++c) {
                if (s[1 + 2 * c] != hd->id[c]) JPG_FAIL(SPE_JPEG_UNSUPPORTED, JR_SCANS);       // another component order
                hd->td[c] = s[2 + 2 * c] >> 4;
                hd->ta[c] = s[2 + 2 * c] & 15;
                if (hd->td[c] > 3 || hd->ta[c] > 3) JPG_FAIL(SPE_JPEG_CORRUPT, JR_HEADER);
            }
            if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0) JPG_FAIL(SPE_JPEG_CORRUPT, JR_HEADER);
            hd->scan = p;
            break;
        }
    }
    if (hd->ncomp == 3) {
        if (adobe && transform != 1) JPG_FAIL(SPE_JPEG_UNSUPPORTED, JR_ADOBE);
        if (!jfif && !adobe && hd->id[0] == 'R' && hd->id[1] == 'G' && hd->id[2] == 'B') JPG_FAIL(SPE_JPEG_UNSUPPORTED, JR_RGB_IDS);
        const bool luma = (hd->h[0] == 1 && hd->v[0] == 1) || (hd->h[0] == 2 && hd->v[0] == 1) || (hd->h[0] == 2 && hd->v[0] == 2);
        if (!luma || hd->h[1] != 1 || hd->v[1] != 1 || hd->h[2] != 1 || hd->v[2] != 1) JPG_FAIL(SPE_JPEG_UNSUPPORTED, JR_SAMPLING);
    } else {
        hd->h[0] = hd->v[0] = 1;                     // one component: the scan is not interleaved, an MCU is one block
    }
    for (int c = 0; c < hd->ncomp; ++c)
        if (!hd->qt_defined[hd->tq[c]] || !hd->huff[0][hd->td[c]].defined || !hd->huff[1][hd->ta[c]].defined)
            JPG_FAIL(SPE_JPEG_CORRUPT, JR_NO_TABLE);
    // a block costs at least two bits, a DC code and an end of block: a frame that the bytes behind the scan header cannot fill is
    // refused here, before anybody allocates 128 bytes a block for a size field a hostile file made up
    const long hm = hd->h[0], vm = hd->v[0];
    const long mcus = (long)((hd->width + 8 * hm - 1) / (8 * hm)) * ((hd->height + 8 * vm - 1) / (8 * vm));
    if (mcus * (hd->ncomp == 1 ? 1 : hm * vm + 2) > 4 * (n - hd->scan)) JPG_FAIL(SPE_JPEG_CORRUPT, JR_TRUNCATED);
    return 0;
}

static inline void spe_jpeg_fill_info(const spe_jpeg_header* hd, int* info) {
    memset(info, 0, sizeof(int) * SPE_JPEG_INFO_INTS);
    const int hmax = hd->h[0], vmax = hd->v[0];      // chroma is 1 x 1
    const int mcux = (hd->width + 8 * hmax - 1) / (8 * hmax), mcuy = (hd->height + 8 * vmax - 1) / (8 * vmax);
    info[JI_WIDTH] = hd->width; info[JI_HEIGHT] = hd->height; info[JI_NCOMP] = hd->ncomp;
    info[JI_HMAX] = hmax; info[JI_VMAX] = vmax; info[JI_RESTART] = hd->restart; info[JI_MCUX] = mcux; info[JI_MCUY] = mcuy;
    info[JI_SCAN] = (int)hd->scan;
    for (int c = 0; c < hd->ncomp; ++c) {
        info[JI_H + c] = hd->h[c]; info[JI_V + c] = hd->v[c];
        info[JI_BW + c] = mcux * hd->h[c]; info[JI_BH + c] = mcuy * hd->v[c];
        info[JI_NBLK + c] = info[JI_BW + c] * info[JI_BH + c];             // <= 8192 * 8192
        info[JI_BLOCKS] += info[JI_NBLK + c];
        for (int k = 0; k < 64; ++k) info[JI_QT + 64 * c + k] = hd->qt[hd->tq[c]][k];
    }
}

// C-ABI: see include/spe_hip.h (spe_jpeg_probe)
static inline int spe_jpeg_probe_impl(const unsigned char* data, long n, int* info) {
    if (!info) return -2;
    spe_jpeg_header hd;
    int reason;
    const int rc = spe_jpeg_parse(data, n, &hd, &reason);
    if (rc) {
        memset(info, 0, sizeof(int) * SPE_JPEG_INFO_INTS);
        info[JI_REASON] = reason;
        return rc;
    }
    spe_jpeg_fill_info(&hd, info);
    return 0;
}

// ---- Huffman decoding: a 9-bit lookahead table, the canonical-code walk for longer codes ---------------------------------------
#define JPG_LOOK 9
struct spe_jpeg_huff {
    uint16_t look[1 << JPG_LOOK];       // (length << 8) | symbol of the code the next 9 bits begin with; 0: longer than 9 bits
    int16_t fast[1 << JPG_LOOK];        // AC tables: (value << 8) | (run << 4) | bits when a code and its value bits fit in 9 bits; else 0
    int maxcode[17], valoff[17], nsym;  // per length: the largest code (-1: none), symbol index of code 0
    unsigned char symbols[256];
};

static inline int spe_jpeg_build(const spe_jpeg_rawhuff* raw, spe_jpeg_huff* h) {
    memset(h->look, 0, sizeof(h->look));
    memcpy(h->symbols, raw->symbols, 256);
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        const int cnt = raw->counts[l - 1];
        h->valoff[l] = k - code;
        if (code + cnt > (1 << l)) return SPE_JPEG_CORRUPT;                  // more codes than the length has
        if (l <= JPG_LOOK)
            for (int i = 0; i < cnt; ++i) {
                const int lo = (code + i) << (JPG_LOOK - l);
                for (int j = 0; j < (1 << (JPG_LOOK - l)); ++j) h->look[lo + j] = (uint16_t)((l << 8) | raw->symbols[k + i]);
            }
        code += cnt;
        k += cnt;
        h->maxcode[l] = cnt ? code - 1 : -1;
        code <<= 1;
    }
    h->nsym = k;
    // a short code followed by a short value, as low-frequency AC coefficients mostly are, decodes with one lookup
    for (int i = 0; i < (1 << JPG_LOOK); ++i) {
        h->fast[i] = 0;
        const int len = h->look[i] >> 8, run = (h->look[i] >> 4) & 15, mag = h->look[i] & 15;
        if (!len || !mag || len + mag > JPG_LOOK) continue;
        int v = ((i << len) & ((1 << JPG_LOOK) - 1)) >> (JPG_LOOK - mag);
        if (v < (1 << (mag - 1))) v -= (1 << mag) - 1;
        if (v >= -128 && v <= 127) h->fast[i] = (int16_t)(v * 256 + run * 16 + len + mag);
    }
    return 0;
}

struct spe_jpeg_bits {
    const unsigned char *p, *end;
    uint64_t buf;
    int bits, pad;                      // bits in buf; how many of them (the lowest) are zeros supplied past a marker or the end
    bool stop;
    // at least 33 bits afterwards: a code (up to 16) and its value (up to 15) never need another fill
    inline void fill() {
        if (bits > 32) return;
        if (!stop && end - p >= 4) {                                          // four bytes at once unless one of them is FF
            const uint32_t w = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
            const uint32_t inv = ~w;
            if (!((inv - 0x01010101u) & ~inv & 0x80808080u)) {
                buf = (buf << 32) | w;
                bits += 32;
                p += 4;
                return;
            }
        }
        while (bits <= 56) {
            unsigned b = 0;
            if (!stop && p < end) {
                b = *p;
                if (b != 0xFF) ++p;
                else if (p + 1 < end && p[1] == 0) p += 2;                   // a stuffed FF 00
                else { stop = true; b = 0; }                                  // a marker, or a lone FF at the end: stays where it is
            } else stop = true;
            if (stop) pad += 8;
            buf = (buf << 8) | b;
            bits += 8;
        }
    }
    inline unsigned peek(int k) const { return (unsigned)(buf >> (bits - k)) & ((1u << k) - 1u); }
    inline bool overrun() const { return bits < pad; }
    // the next symbol, -1 for an undefined code.  fill() must have run just before: 33 bits are there.
    inline int decode(const spe_jpeg_huff& h) {
        const unsigned e = h.look[peek(JPG_LOOK)];
        if (e >> 8) { bits -= (int)(e >> 8); return (int)(e & 255u); }
        const unsigned w = peek(16);
        for (int l = JPG_LOOK + 1; l <= 16; ++l) {
            const int c = (int)(w >> (16 - l));
            if (c <= h.maxcode[l]) {
                const int idx = h.valoff[l] + c;
                if (idx < 0 || idx >= h.nsym) return -1;
                bits -= l;
                return h.symbols[idx];
            }
        }
        return -1;
    }
    inline int receive_extend(int s) {
        const int v = (int)peek(s);
        bits -= s;
        return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
    }
};

// C-ABI: see include/spe_hip.h (spe_jpeg_entropy)
static inline int spe_jpeg_entropy_impl(const unsigned char* data, long n, short* coef, long coef_elems, int* reason_out) {
    spe_jpeg_header hd;
    int reason_local, info[SPE_JPEG_INFO_INTS];
    int* reason = reason_out ? reason_out : &reason_local;
    const int rc = spe_jpeg_parse(data, n, &hd, reason);
    if (rc) return rc;
    spe_jpeg_fill_info(&hd, info);
    if (!coef || coef_elems < (long)info[JI_BLOCKS] * 64) JPG_FAIL(-2, JR_BUFFER);
    spe_jpeg_huff dc[3], ac[3];
    for (int c = 0; c < hd.ncomp; ++c)
        if (spe_jpeg_build(&hd.huff[0][hd.td[c]], &dc[c]) || spe_jpeg_build(&hd.huff[1][hd.ta[c]], &ac[c]))
            JPG_FAIL(SPE_JPEG_CORRUPT, JR_BAD_CODE);
    long base[3] = {0, (long)info[JI_NBLK], (long)info[JI_NBLK] + info[JI_NBLK + 1]};
    spe_jpeg_bits br = {data + hd.scan, data + n, 0, 0, 0, false};
    int pred[3] = {0, 0, 0};
    const int mcux = info[JI_MCUX], mcuy = info[JI_MCUY];
    int togo = hd.restart, rst = 0;
    for (int my = 0; my < mcuy; ++my)
        for (int mx = 0; mx < mcux; ++mx) {
            if (hd.restart && togo == 0) {                                    // byte-align, take the marker, start over
                // only the padding of the last byte may be left: whole unread bytes in front of the marker are refused here, so the
                // verdict does not depend on how far ahead the reader happened to have read
                if (br.bits - br.pad >= 8) JPG_FAIL(SPE_JPEG_CORRUPT, JR_RESTART);
                br.buf = 0; br.bits = 0; br.pad = 0; br.stop = false;
                if (br.p >= br.end) JPG_FAIL(SPE_JPEG_CORRUPT, JR_TRUNCATED);
                if (*br.p != 0xFF) JPG_FAIL(SPE_JPEG_CORRUPT, JR_RESTART);
                while (br.p < br.end && *br.p == 0xFF) ++br.p;
                if (br.p >= br.end) JPG_FAIL(SPE_JPEG_CORRUPT, JR_TRUNCATED);
                if (*br.p != 0xD0 + (rst & 7)) JPG_FAIL(SPE_JPEG_CORRUPT, JR_RESTART);
                ++br.p;
                ++rst;
                togo = hd.restart;
                pred[0] = pred[1] = pred[2] = 0;
            }
            for (int c = 0; c < hd.ncomp; ++c)
                for (int by = 0; by < hd.v[c]; ++by)
                    for (int bx = 0; bx < hd.h[c]; ++bx) {
                        short* blk = coef + (base[c] + (long)(my * hd.v[c] + by) * info[JI_BW + c] + (mx * hd.h[c] + bx)) * 64;
                        memset(blk, 0, 128);
                        br.fill();
                        int s = br.decode(dc[c]);
                        if (s < 0 || s > 15) JPG_FAIL(SPE_JPEG_CORRUPT, JR_BAD_CODE);
                        if (s) pred[c] += br.receive_extend(s);
                        pred[c] = (short)pred[c];                              // hostile sums stay in range; real ones fit in 12 bits
                        blk[0] = (short)pred[c];
                        for (int k = 1; k < 64;) {
                            br.fill();
                            const int f = ac[c].fast[br.peek(JPG_LOOK)];
                            if (f) {                                          // run, size and value in one lookup
                                k += (f >> 4) & 15;
                                if (k > 63) JPG_FAIL(SPE_JPEG_CORRUPT, JR_RUN);
                                br.bits -= f & 15;
                                blk[spe_jpeg_natural[k++]] = (short)(f >> 8);
                                continue;
                            }
                            const int rs = br.decode(ac[c]);
                            if (rs < 0) JPG_FAIL(SPE_JPEG_CORRUPT, JR_BAD_CODE);
                            const int r = rs >> 4;
                            s = rs & 15;
                            if (s == 0) {
                                if (r != 15) break;                           // end of block
                                k += 16;
                                if (k > 64) JPG_FAIL(SPE_JPEG_CORRUPT, JR_RUN);
                                continue;
                            }
                            k += r;
                            if (k > 63) JPG_FAIL(SPE_JPEG_CORRUPT, JR_RUN);
                            blk[spe_jpeg_natural[k]] = (short)br.receive_extend(s);
                            ++k;
                        }
                    }
            if (br.overrun()) JPG_FAIL(SPE_JPEG_CORRUPT, JR_TRUNCATED);
            --togo;
        }
    return 0;
}
#endif /* SPE_JPEG_ENTROPY_H */
