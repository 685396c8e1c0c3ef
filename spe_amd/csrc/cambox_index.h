// Index arithmetic of the labelling form of the CAM -> box step (csrc/cambox_labels.hip), shared with the serial host
// restatement tools/micro/cambox_host.hip, which runs it under the host sanitizers.  Everything here is integer arithmetic
// on the zero-padded image: (rows + 2) x (cols + 2) pixels, width W = cols + 2, pixel (y, x) at index y * W + x, the image
// itself at 1 <= y <= rows, 1 <= x <= cols.
//
// Formulation (every quantity of a Suzuki-Abe border walk without the walk):
//   labels  foreground 8-connected, background 4-connected, label = index of the component's raster-first pixel; background
//           label 0 is the frame, every other background component is a hole;
//   borders one outer border per foreground component, one hole border per hole (cv2.findContours RETR_TREE);
//   area2   (shoelace area in half units) per 2x2 window ("cell"): the cell's foreground component gets 2 when the cell has
//           4 foreground pixels and 1 when it has 3; every hole with k >= 1 pixels in the cell gets 2 when k >= 2, else 1;
//           these sums are each border's OWN count;
//   parent  of a hole: the foreground component of the pixel west of the hole's raster-first pixel; of a component: the hole
//           that holds the pixel west of its raster-first pixel (the frame there: no parent) - in both cases the label of the
//           pixel at index root - 1, always smaller than the root;
//   area2   of a border = its own count + the own counts of every border below it in that tree (the polygon of a border encloses
//           its holes, their islands, the holes of those ...): every node adds its own count to each of its ancestors;
//   box     outer: the box of the component's pixels; hole: the box of the hole's pixels grown by one on every side;
//   key     (discovery position of the raster scan) outer: the component's label; hole: its label - 1.
#pragma once

#ifndef __HIPCC__
#define __host__
#define __device__
#endif
#define CAMBOX_HD __host__ __device__ inline

#define CAMBOX_MAX_BOXES 2048        // cap of max_boxes: area and key of every survivor in the rank kernel's LDS (16 KiB)
#define CAMBOX_STATUS_OVERFLOW (-5)  // more than max_boxes survivors (the status of the host path)
#define CAMBOX_STATUS_CHAIN (-6)     // a label chain longer than the pixel count: the merge gave up instead of spinning

// ints per map of the workspace: label, own2, area2, x0, y0, x1, y1 over the padded image (rounded up to 4 pixels), 4 flag words,
// the survivor list (6 ints each: area2, key, box)
CAMBOX_HD long cambox_padded_pixels(int rows, int cols) { return (long)(rows + 2) * (cols + 2); }
CAMBOX_HD long cambox_plane_ints(int rows, int cols) { return (cambox_padded_pixels(rows, cols) + 3) & ~3L; }
CAMBOX_HD long cambox_map_ints(int rows, int cols) { return 7 * cambox_plane_ints(rows, cols) + 4 + 6 * CAMBOX_MAX_BOXES; }

// foreground test of padded pixel (y, x) on the unpadded image img[rows][cols]; the padding is background
CAMBOX_HD bool cambox_fg(const unsigned char* img, int rows, int cols, int y, int x) {
    return y >= 1 && y <= rows && x >= 1 && x <= cols && img[(long)(y - 1) * cols + (x - 1)] != 0;
}

// first lane of the run of set bits of `same` that contains bit `lane` (bit `lane` is set): the initial link of a pixel is
// the start of its horizontal run inside its 64-pixel segment
CAMBOX_HD int cambox_run_start(unsigned long long same, int lane) {
    const unsigned long long below = ~same & ((1ull << lane) - 1ull);       // cleared bits under the lane
    return below ? 64 - __builtin_clzll(below) : 0;                           // one past the highest of them
}

// The unions pixel p = (y, x) owes to its raster-earlier neighbours, as index offsets from p (0 = none), given the classes
// of W, NW, N, NE relative to p's own class (true = same class).  Foreground (8-connected): N alone covers NW and NE, which
// touch N in their own row; W covers NW.  A union is skipped when W already owes it: W, in p's run, reaches N as its NE and
// NW as its N.  Background (4-connected): N, unless W is in the run and NW continues the run above.
struct CamboxLinks { int n; int off[3]; };
CAMBOX_HD CamboxLinks cambox_links(bool fg, bool w, bool nw, bool n, bool ne, int W) {
    CamboxLinks l; l.n = 0; l.off[0] = l.off[1] = l.off[2] = 0;
    if (fg) {
        if (n) { if (!w) l.off[l.n++] = -W; }
        else {
            if (nw && !w) l.off[l.n++] = -W - 1;
            if (ne) l.off[l.n++] = -W + 1;
        }
    } else if (n && !(w && nw)) l.off[l.n++] = -W;
    return l;
}

// Half-unit contributions of one cell.  lab[4] / fg[4]: labels and classes of (y, x), (y, x+1), (y+1, x), (y+1, x+1).
// own: the foreground component (-1: none) and its increment; hole[0..1]: up to two distinct holes (a cell touches two
// only across a diagonal) and their increments; the frame (label 0) takes nothing.
struct CamboxCell { int own, own_add; int hole[2], hole_add[2]; };
CAMBOX_HD CamboxCell cambox_cell(const int lab[4], const bool fg[4]) {
    CamboxCell c; c.own = -1; c.own_add = 0; c.hole[0] = c.hole[1] = -1; c.hole_add[0] = c.hole_add[1] = 0;
    int nfg = 0;
    for (int k = 0; k < 4; ++k) if (fg[k]) { ++nfg; c.own = lab[k]; }
    c.own_add = nfg == 4 ? 2 : (nfg == 3 ? 1 : 0);
    if (!c.own_add) c.own = -1;
    int nh = 0;
    for (int k = 0; k < 4; ++k) {
        if (fg[k] || lab[k] == 0) continue;
        bool seen = false;
        for (int j = 0; j < k; ++j) seen = seen || (!fg[j] && lab[j] == lab[k]);
        if (seen) continue;
        int cnt = 0;
        for (int j = k; j < 4; ++j) cnt += (!fg[j] && lab[j] == lab[k]) ? 1 : 0;
        if (nh < 2) { c.hole[nh] = lab[k]; c.hole_add[nh] = cnt >= 2 ? 2 : 1; ++nh; }
    }
    return c;
}

// discovery key of the border of root pixel `root`
CAMBOX_HD int cambox_key(int root, bool fg) { return fg ? root : root - 1; }

// emitted box [x, y, x + w, y + h] in unpadded coordinates from the padded inclusive box of the component's pixels
CAMBOX_HD void cambox_emit(bool fg, int px0, int py0, int px1, int py1, int out[4]) {
    const int grow = fg ? 0 : 1;
    out[0] = px0 - 1 - grow; out[1] = py0 - 1 - grow; out[2] = px1 + grow; out[3] = py1 + grow;
}

// selection: a border survives when area >= top * area_ratio in double (area = area2 / 2), the expression of the host path
CAMBOX_HD bool cambox_keep(int area2, int top2, float area_ratio) {
    return (double)area2 * 0.5 >= ((double)top2 * 0.5) * (double)area_ratio;
}
// a ranks before b: area descending, discovery key ascending (the stable sort of the host path)
CAMBOX_HD bool cambox_before(int area2_a, int key_a, int area2_b, int key_b) {
    return area2_a > area2_b || (area2_a == area2_b && key_a < key_b);
}
