/* The oracle's per-step trace (oracle/pv_oracle.c pvo_get_phase_trace) as a stand-alone program, for ASan + UBSan:
 * a stereo run long enough for the trace buffer to grow several times, read back whole, in part and with max = 0.
 * The input has a stretch of exact zeros in one channel, so all three branches occur. */
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
    free(part); free(npk); free(mode);
    for (int c = 0; c < CH; ++c) { free(x[c]); free(y[c]); }
    pvo_destroy(h);
    printf("oracle trace: %ld steps (%ld init, %ld prop, %ld lock), %d failures\n", n, count[0], count[1], count[2], failures);
    return failures ? 1 : 0;
}
