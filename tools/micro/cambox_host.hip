// Serial host restatement of the labelling form of the CAM -> box step, on the index arithmetic the kernels use
// (spe_amd/csrc/cambox_index.h): same padded offsets, run starts, union rules, cell windows, hole keys and ranking, one
// pixel at a time.  It touches no GPU; it exists so that this arithmetic runs under the HOST sanitizers:
//
//   hipcc --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -I spe_amd/csrc tools/micro/cambox_host.hip -o cambox_host
//   ./cambox_host cases.txt
//
// cases.txt: per case one line `name rows cols area_ratio max_boxes`, then `rows` lines of `cols` characters '0' / '1'.
// Output per case: `case name nborders status nboxes`, then nborders lines `b area2 x0 y0 x1 y1` (inclusive box, discovery
// order), then nboxes lines `s x0 y0 x1 y1` (the selection, [x, y, x+w, y+h]).  tests/test_cambox_ref_cpu.py compares both
// with oracle/cam_oracle.py.
#include "cambox_index.h"
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

namespace {
int find_root(const std::vector<int>& lab, int a) {
    while (lab[(size_t)a] != a) a = lab[(size_t)a];
    return a;
}
void unite(std::vector<int>& lab, int a, int b) {
    a = find_root(lab, a); b = find_root(lab, b);
    if (a == b) return;
    if (a < b) std::swap(a, b);
    lab[(size_t)a] = b;                                     // what atomicMin on a root leaves
}

struct Border { int key, area2, box[4]; bool fg; };

int run_case(const std::string& name, int rows, int cols, float ratio, int max_boxes, const std::vector<unsigned char>& img) {
    const int W = cols + 2, Hh = rows + 2;
    const long npix = cambox_padded_pixels(rows, cols);
    std::vector<int> lab((size_t)npix), own2((size_t)npix, 0), area2((size_t)npix, 0), x0((size_t)npix, INT_MAX), y0((size_t)npix, INT_MAX), x1((size_t)npix, -1),
        y1((size_t)npix, -1);
    const unsigned char* im = img.data();
    // init: run starts inside 64-pixel segments
    for (int y = 0; y < Hh; ++y)
        for (int s = 0; s < W; s += 64) {
            unsigned long long fm = 0, vm = 0;
            for (int l = 0; l < 64 && s + l < W; ++l) { vm |= 1ull << l; if (cambox_fg(im, rows, cols, y, s + l)) fm |= 1ull << l; }
            for (int l = 0; l < 64 && s + l < W; ++l) {
                const bool fg = (fm >> l) & 1;
                lab[(size_t)y * W + s + l] = y * W + s + cambox_run_start(fg ? fm : (vm & ~fm), l);
            }
        }
    // merge
    for (int y = 0; y < Hh; ++y)
        for (int x = 0; x < W; ++x) {
            const int p = y * W + x;
            const bool fg = cambox_fg(im, rows, cols, y, x);
            const bool w = x > 0 && cambox_fg(im, rows, cols, y, x - 1) == fg;
            if (x % 64 == 0 && w) unite(lab, p, p - 1);
            if (y == 0) continue;
            const bool nw = x > 0 && cambox_fg(im, rows, cols, y - 1, x - 1) == fg;
            const bool n = cambox_fg(im, rows, cols, y - 1, x) == fg;
            const bool ne = x < W - 1 && cambox_fg(im, rows, cols, y - 1, x + 1) == fg;
            const CamboxLinks l = cambox_links(fg, w, nw, n, ne, W);
            for (int k = 0; k < l.n; ++k) unite(lab, p, p + l.off[k]);
        }
    // compress
    for (long p = 0; p < npix; ++p) lab[(size_t)p] = find_root(lab, (int)p);
    // count
    for (int y = 0; y < Hh - 1; ++y)
        for (int x = 0; x < W - 1; ++x) {
            const int p = y * W + x;
            const int l4[4] = {lab[(size_t)p], lab[(size_t)p + 1], lab[(size_t)p + W], lab[(size_t)p + W + 1]};
            const bool f4[4] = {cambox_fg(im, rows, cols, y, x), cambox_fg(im, rows, cols, y, x + 1), cambox_fg(im, rows, cols, y + 1, x),
                                cambox_fg(im, rows, cols, y + 1, x + 1)};
            const CamboxCell c = cambox_cell(l4, f4);
            if (c.own >= 0) own2[(size_t)c.own] += c.own_add;
            for (int k = 0; k < 2; ++k) if (c.hole[k] >= 0) own2[(size_t)c.hole[k]] += c.hole_add[k];
            if (f4[0] || l4[0] != 0) {
                const bool me = f4[0];
                if (f4[1] != me || f4[2] != me || cambox_fg(im, rows, cols, y, x - 1) != me || cambox_fg(im, rows, cols, y - 1, x) != me) {
                    const size_t r = (size_t)l4[0];
                    x0[r] = std::min(x0[r], x); y0[r] = std::min(y0[r], y); x1[r] = std::max(x1[r], x); y1[r] = std::max(y1[r], y);
                }
            }
        }
    // fold: every border counts for itself and for each of its ancestors (parent = label of the pixel west of the root)
    for (long p = 1; p < npix; ++p) {
        if (lab[(size_t)p] != p) continue;
        area2[(size_t)p] += own2[(size_t)p];
        for (int a = lab[(size_t)p - 1]; a != 0; a = lab[(size_t)a - 1]) area2[(size_t)a] += own2[(size_t)p];
    }
    // select
    std::vector<Border> bs;
    int top = -1;
    for (long p = 1; p < npix; ++p) {
        if (lab[(size_t)p] != p) continue;
        Border b;
        b.fg = cambox_fg(im, rows, cols, (int)(p / W), (int)(p % W));
        b.key = cambox_key((int)p, b.fg); b.area2 = area2[(size_t)p];
        cambox_emit(b.fg, x0[(size_t)p], y0[(size_t)p], x1[(size_t)p], y1[(size_t)p], b.box);
        top = std::max(top, b.area2);
        bs.push_back(b);
    }
    std::sort(bs.begin(), bs.end(), [](const Border& a, const Border& b) { return a.key < b.key; });
    std::vector<const Border*> keep;
    for (const Border& b : bs) if (cambox_keep(b.area2, top, ratio)) keep.push_back(&b);
    int status = 0;
    std::vector<std::vector<int>> out;
    if (bs.empty()) out.push_back({0, 0, 1, 1});
    else if ((long)keep.size() > max_boxes) status = CAMBOX_STATUS_OVERFLOW;
    else {
        out.resize(keep.size());
        for (size_t s = 0; s < keep.size(); ++s) {
            size_t rank = 0;
            for (size_t t = 0; t < keep.size(); ++t) rank += cambox_before(keep[t]->area2, keep[t]->key, keep[s]->area2, keep[s]->key) ? 1 : 0;
            out[rank] = {keep[s]->box[0], keep[s]->box[1], keep[s]->box[2], keep[s]->box[3]};
        }
    }
    std::printf("case %s %zu %d %zu\n", name.c_str(), bs.size(), status, out.size());
    for (const Border& b : bs) std::printf("b %d %d %d %d %d\n", b.area2, b.box[0], b.box[1], b.box[2] - 1, b.box[3] - 1);
    for (const auto& o : out) std::printf("s %d %d %d %d\n", o[0], o[1], o[2], o[3]);
    return 0;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s cases.txt\n", argv[0]); return 2; }
    FILE* f = std::fopen(argv[1], "r");
    if (!f) { std::perror(argv[1]); return 2; }
    char name[256];
    int rows, cols, max_boxes;
    float ratio;
    int ncases = 0;
    while (std::fscanf(f, "%255s %d %d %f %d", name, &rows, &cols, &ratio, &max_boxes) == 5) {
        if (rows < 1 || cols < 1 || cambox_padded_pixels(rows, cols) > (1L << 30)) { std::fprintf(stderr, "bad shape in case %s\n", name); return 2; }
        std::vector<unsigned char> img((size_t)rows * cols);
        std::vector<char> line((size_t)cols + 2);
        for (int y = 0; y < rows; ++y) {
            char fmt[32];
            std::snprintf(fmt, sizeof fmt, "%%%ds", cols);
            if (std::fscanf(f, fmt, line.data()) != 1) { std::fprintf(stderr, "short case %s\n", name); return 2; }
            for (int x = 0; x < cols; ++x) {
                if (line[(size_t)x] != '0' && line[(size_t)x] != '1') { std::fprintf(stderr, "bad pixel in case %s\n", name); return 2; }
                img[(size_t)y * cols + x] = line[(size_t)x] == '1' ? 255 : 0;
            }
        }
        run_case(name, rows, cols, ratio, max_boxes, img);
        ++ncases;
    }
    std::fclose(f);
    std::printf("done %d\n", ncases);
    return 0;
}
