/* The oracle's per-step trace (oracle/pv_oracle.c pvo_get_phase_trace) as a stand-alone program, for ASan + UBSan:
 * a stereo run long enough for the trace buffer to grow several times, read back whole, in part and with max = 0.
 * The input has a stretch of exact zeros in one channel, so all three branches occur.  Then the opt-in plane trace
 * (pvo_enable_plane_trace / pvo_get_plane_trace) on a second handle. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pv_oracle.h"

int main(void) {
    enum { CH = 2, FRAMES = 200000, BLOCK = 480 };
    pvo_config cfg = {48000, CH, 1.0f, 4.0f, PVO_NORMAL_SHIFT, PVO_PHASE_LOCKED, 512, 0};
    pvo *h = pvo_create(&cfg);
    if (!h) return 2;
    float *x[CH], *y[CH];
    unsigned s = 12345u;
    for (int c = 0; c < CH; ++c) {
        x[c] = (float *)malloc(sizeof(float) * FRAMES);
        y[c] = (float *)malloc(sizeof(float) * 65536);
        for (int i = 0; i < FRAMES; ++i) {
            s = s * 1664525u + 1013904223u;
            x[c][i] = (float)((int)(s >> 16) - 32768) / 65536.0f;
        }
    }
    memset(x[0] + 50000, 0, sizeof(float) * 2000);
    int failures = 0;
    if (pvo_get_phase_trace(h, NULL, NULL, 0) != 0) ++failures;
    for (int i = 0; i < FRAMES; i += BLOCK) {
        const float *in[CH] = {x[0] + i, x[1] + i};
        int n = FRAMES - i < BLOCK ? FRAMES - i : BLOCK;
        int got = pvo_process(h, in, n);
        if (got < 0) return 3;
        while (got > 0) {
            int take = got < 65536 ? got : 65536;
            got -= pvo_retrieve(h, y, take);
        }
    }
    pvo_info info;
    pvo_get_info(h, &info);
    const long n = pvo_get_phase_trace(h, NULL, NULL, 0);
    if (n != info.slices * CH || n < 4096) ++failures; /* (the buffer starts at 1024 entries and doubles) */
    int *npk = (int *)malloc(sizeof(int) * n), *mode = (int *)malloc(sizeof(int) * n);
    if (pvo_get_phase_trace(h, npk, mode, n) != n) ++failures;
    long count[3] = {0, 0, 0};
    const int cap = (256 - 4 + 2) / 3;
    for (long i = 0; i < n; ++i) {
        if (mode[i] < 0 || mode[i] > 2 || npk[i] < 0 || npk[i] > cap) { ++failures; break; }
        ++count[mode[i]];
    }
    if (count[PVO_TRACE_INIT] != 1 || mode[0] != PVO_TRACE_INIT || count[PVO_TRACE_PROP] < 2 || count[PVO_TRACE_LOCK] < n / 2) ++failures;
    /* a partial read copies `max` entries and still reports all of them; an exactly sized buffer is not overrun */
    int *part = (int *)malloc(sizeof(int) * 7);
    if (pvo_get_phase_trace(h, part, NULL, 7) != n || memcmp(part, npk, sizeof(int) * 7)) ++failures;
    if (pvo_get_phase_trace(h, NULL, part, 7) != n || memcmp(part, mode, sizeof(int) * 7)) ++failures;
    free(part);
    /* the planes were never switched on for this handle, and cannot be once steps exist */
    if (pvo_get_plane_trace(h, 0, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL) != -1) ++failures;
    if (pvo_enable_plane_trace(h) != -1) ++failures;
    pvo_destroy(h);

    /* the plane trace (pvo_enable_plane_trace / pvo_get_plane_trace): the same input through a second handle with the
     * planes on -- the buffers grow several times from 64 steps -- read back whole, one plane at a time, in part, past
     * the end and with nothing asked for; the counts and modes must be the first run's */
    enum { H = 257, PART = 20000 };
    h = pvo_create(&cfg);
    if (!h) return 2;
    if (pvo_enable_plane_trace(h) != 0) ++failures;
    if (pvo_get_plane_trace(h, 0, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL) != 0) ++failures;
    for (int i = 0; i < PART; i += BLOCK) {
        const float *in[CH] = {x[0] + i, x[1] + i};
        int n2 = PART - i < BLOCK ? PART - i : BLOCK;
        int got = pvo_process(h, in, n2);
        if (got < 0) return 3;
        while (got > 0) {
            int take = got < 65536 ? got : 65536;
            got -= pvo_retrieve(h, y, take);
        }
    }
    const long m = pvo_get_phase_trace(h, NULL, NULL, 0);
    if (m < 512 || m > n) ++failures;
    int *npk2 = (int *)malloc(sizeof(int) * m), *mode2 = (int *)malloc(sizeof(int) * m);
    pvo_get_phase_trace(h, npk2, mode2, m);
    if (memcmp(npk2, npk, sizeof(int) * m) || memcmp(mode2, mode, sizeof(int) * m)) ++failures;
    float *pl[6];
    for (int w = 0; w < 6; ++w) pl[w] = (float *)malloc(sizeof(float) * H * m);
    int *peaks = (int *)malloc(sizeof(int) * H * m);
    if (pvo_get_plane_trace(h, 0, m, pl[0], pl[1], pl[2], pl[3], peaks, pl[4], pl[5]) != m) ++failures;
    long bad = 0;
    for (long s2 = 0; s2 < m; ++s2) {
        const float *re = pl[0] + s2 * H, *im = pl[1] + s2 * H, *mag = pl[2] + s2 * H, *rot = pl[4] + s2 * H;
        const int *pk = peaks + s2 * H;
        for (int i = 0; i < H; ++i)
            if (!(mag[i] >= 0) || (re[i] == 0 && im[i] == 0) != (mag[i] == 0)) ++bad;
        for (int i = 0; i < npk2[s2]; ++i)
            if (pk[i] < 2 || pk[i] > H - 4 || (i && pk[i] < pk[i - 1] + 3)) ++bad;
        for (int i = npk2[s2]; i < H; ++i)
            if (pk[i] != 0 || rot[i] != 0) ++bad;
        if (mode2[s2] != PVO_TRACE_LOCK)
            for (int i = 0; i < npk2[s2]; ++i)
                if (rot[i] != 0) ++bad;
        if (pl[5][s2 * H + H - 1] != 0) ++bad;
    }
    if (bad) ++failures;
    /* the first step's output phases are its analysis phases */
    if (memcmp(pl[5], pl[3], sizeof(float) * (H - 1))) ++failures;
    /* one plane at a time, a window in the middle, into exactly sized buffers */
    float *one = (float *)malloc(sizeof(float) * H * 3);
    int *onep = (int *)malloc(sizeof(int) * H * 3);
    if (pvo_get_plane_trace(h, 100, 3, NULL, NULL, one, NULL, NULL, NULL, NULL) != m ||
        memcmp(one, pl[2] + 100 * H, sizeof(float) * H * 3)) ++failures;
    if (pvo_get_plane_trace(h, 100, 3, NULL, NULL, NULL, NULL, onep, NULL, NULL) != m ||
        memcmp(onep, peaks + 100 * H, sizeof(int) * H * 3)) ++failures;
    /* a window that runs past the end is clipped: the last step only; one that starts past it copies nothing */
    memset(one, 0, sizeof(float) * H * 3);
    if (pvo_get_plane_trace(h, m - 1, 3, NULL, NULL, NULL, one, NULL, NULL, NULL) != m ||
        memcmp(one, pl[3] + (m - 1) * H, sizeof(float) * H) || one[H] != 0) ++failures;
    if (pvo_get_plane_trace(h, m + 5, 3, one, one, one, one, onep, one, one) != m) ++failures;
    if (pvo_get_plane_trace(h, -1, 3, one, one, one, one, onep, one, one) != m) ++failures;
    free(one); free(onep); free(peaks); free(npk2); free(mode2);
    for (int w = 0; w < 6; ++w) free(pl[w]);
    free(npk); free(mode);
    for (int c = 0; c < CH; ++c) { free(x[c]); free(y[c]); }
    pvo_destroy(h);
    printf("oracle trace: %ld steps (%ld init, %ld prop, %ld lock); plane trace: %ld steps, %ld bad values; %d failures\n",
           n, count[0], count[1], count[2], m, bad, failures);
    return failures ? 1 : 0;
}
