// A stand-alone host program around rg_pixels_host's source (rogue-gym_amd/csrc/rg_pixels.h), built by tests/test_pixels_host.py with
// -fsanitize=address,undefined: every output buffer is allocated at its exact size, so a write past an image, a read past a table or a screen, or a shift
// out of range ends the run.  It also restates the rule pixel by pixel and compares.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rg_pixels.h"

static uint32_t rnd_state = 12345u;
static uint32_t rnd() { rnd_state = rnd_state * 1664525u + 1013904223u; return rnd_state >> 8; }

static int check(int th, int channels, int H, int W, int cy, int cx, int ry, int rx) {
    std::vector<uint8_t> font(256 * (size_t)th), pal(257 * 3), screen((size_t)H * W);
    for (auto &b : font) b = (uint8_t)rnd();
    for (auto &b : pal) b = (uint8_t)rnd();
    for (auto &b : screen) b = (uint8_t)rnd();
    font[0x20 * th] |= 0x81;
    const int hc = ry < 0 ? H : 2 * ry + 1, wc = ry < 0 ? W : 2 * rx + 1, y0 = ry < 0 ? 0 : cy - ry, x0 = ry < 0 ? 0 : cx - rx;
    std::vector<uint8_t> out((size_t)channels * hc * th * wc * 8);
    std::string err;
    if (rg_px_host(err, th, font.data(), pal.data(), channels, H, W, screen.data(), cy, cx, ry, rx, out.data())) { printf("refused: %s\n", err.c_str()); return 1; }
    for (int c = 0; c < channels; c++)
        for (int py = 0; py < hc * th; py++)
            for (int px = 0; px < wc * 8; px++) {
                const int y = y0 + py / th, x = x0 + px / 8;
                const int g = (y >= 0 && y < H && x >= 0 && x < W) ? screen[(size_t)y * W + x] : ' ';
                const int ink = (font[g * th + py % th] >> (7 - px % 8)) & 1, e = ink ? g : 256;
                const uint8_t want = channels == 3 ? pal[3 * e + c] : (uint8_t)((77 * pal[3 * e] + 150 * pal[3 * e + 1] + 29 * pal[3 * e + 2] + 128) >> 8);
                if (out[((size_t)c * hc * th + py) * wc * 8 + px] != want) { printf("mismatch th %d C %d %dx%d win (%d,%d) at c %d y %d x %d\n", th, channels, W, H, ry, rx, c, py, px); return 1; }
            }
    return 0;
}

int main() {
    static const int sizes[4][2] = {{16, 32}, {17, 33}, {24, 80}, {33, 97}}, wins[4][2] = {{0, 0}, {5, 5}, {1, 7}, {47, 159}}, ths[3] = {8, 13, 16};
    int bad = 0, runs = 0;
    for (int th : ths)
        for (int channels = 1; channels <= 3; channels += 2) {
            for (auto &s : sizes) { bad += check(th, channels, s[0], s[1], 0, 0, -1, 0); runs++; }
            for (auto &w : wins) {
                const int H = 17, W = 33, cys[3] = {0, H / 2, H - 1}, cxs[3] = {0, W / 2, W - 1};
                for (int cy : cys) for (int cx : cxs) { bad += check(th, channels, H, W, cy, cx, w[0], w[1]); runs++; }
            }
        }
    // the built-in tileset and the refusals: nothing written
    std::vector<uint8_t> screen(16 * 32, (uint8_t)'#'), out(16 * 8 * 32 * 8, 0xAB);
    std::string err;
    bad += rg_px_host(err, 0, nullptr, nullptr, 1, 16, 32, screen.data(), 0, 0, -1, 0, out.data());
    std::vector<uint8_t> guard(64, 0xAB), font(256 * 16), pal(257 * 3);
    bad += !rg_px_host(err, 7, font.data(), pal.data(), 1, 16, 32, screen.data(), 0, 0, -1, 0, guard.data());
    bad += !rg_px_host(err, 17, font.data(), pal.data(), 1, 16, 32, screen.data(), 0, 0, -1, 0, guard.data());
    bad += !rg_px_host(err, 8, font.data(), pal.data(), 2, 16, 32, screen.data(), 0, 0, -1, 0, guard.data());
    bad += !rg_px_host(err, 8, font.data(), pal.data(), 1, 16, 32, screen.data(), 16, 0, 1, 1, guard.data());
    bad += !rg_px_host(err, 8, font.data(), pal.data(), 1, 16, 32, screen.data(), 0, 0, 48, 1, guard.data());
    for (uint8_t b : guard) bad += b != 0xAB;
    printf("%d runs, %d bad\n", runs, bad);
    return bad ? 1 : 0;
}
