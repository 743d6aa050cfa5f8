/* load_tracking_host_probe.c — what request counting costs the call it rides on: rio_op_lookup answered from the host shadow,
 * 16 caller threads sharing one provider (the string layer's hottest path: no device round trip, ~0.3 us a call).  `reps` timed
 * windows of `calls` lookups per thread over `objects` placed keys, each thread walking the keys from its own offset (all threads
 * meet on the same rows' counters); one JSON line per window.
 *   usage: load_tracking_host_probe <label> <track: 0|1> [objects] [calls] [reps] [threads]
 * Built with -DNO_LOAD_TRACKING against a library that has no rio_op_set_load_tracking (the commit before the feature): the
 * yardstick whose own run-to-run spread the "tracking off" figure must sit in.  tools/load_tracking_host_ab.sh builds and
 * alternates the three. */
#define _POSIX_C_SOURCE 200809L
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "rio_gpu_object_placement.h"

typedef struct { rio_op_t* p; int tid, calls, objects, bad; } job;

static double now_s(void) {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

static void* worker(void* arg) {
    job* j = (job*)arg;
    char id[32], out[64];
    int k, found;
    for (k = 0; k < j->calls; ++k) {
        snprintf(id, sizeof id, "o%d", (j->tid * 997 + k) % j->objects);
        found = 0;
        if (rio_op_lookup(j->p, "Svc", id, out, sizeof out, &found) != RIO_GP_OK || !found) j->bad++;
    }
    return 0;
}

int main(int argc, char** argv) {
    const char* label = argc > 1 ? argv[1] : "run";
    const int track = argc > 2 ? atoi(argv[2]) : 0;
    const int objects = argc > 3 ? atoi(argv[3]) : 20000, calls = argc > 4 ? atoi(argv[4]) : 200000;
    const int reps = argc > 5 ? atoi(argv[5]) : 5, T = argc > 6 ? atoi(argv[6]) : 16;
    rio_op_cfg cfg;
    rio_op_t* p = 0;
    pthread_t th[256];
    job jobs[256];
    char id[32], out[64];
    int i, r, found, bad = 0;
    uint64_t b0 = 0, r0 = 0, b1 = 0, r1 = 0;
    if (T > 256) return 2;
    memset(&cfg, 0, sizeof cfg);
    cfg.struct_size = (uint32_t)sizeof cfg;
    cfg.max_objects = (uint64_t)objects + 16;
    cfg.max_nodes = 8;
    if (rio_op_create(&cfg, &p) != RIO_GP_OK) { fprintf(stderr, "create: %s\n", rio_op_last_error(0)); return 1; }
    for (i = 0; i < 4; ++i) {
        char a[32];
        snprintf(a, sizeof a, "10.0.0.%d:5000", i);
        if (rio_op_set_member(p, a, 1, RIO_GP_CAP_INF)) return 1;
    }
    for (i = 0; i < objects; ++i) {   /* placed and, with that, in the host shadow */
        char a[32];
        snprintf(id, sizeof id, "o%d", i);
        snprintf(a, sizeof a, "10.0.0.%d:5000", i & 3);
        if (rio_op_update(p, "Svc", id, a)) return 1;
    }
    for (i = 0; i < objects; ++i) {   /* (and warm) */
        snprintf(id, sizeof id, "o%d", i);
        if (rio_op_lookup(p, "Svc", id, out, sizeof out, &found) || !found) return 1;
    }
#ifndef NO_LOAD_TRACKING
    if (rio_op_set_load_tracking(p, track)) return 1;
#else
    if (track) return 2;
#endif
    for (r = 0; r < reps + 1; ++r) {  /* (the first window warms the threads' caches: not printed) */
        const struct timespec nap = {0, 150000000};  /* a fresh scheduler period for every window (cgroup cpu.max) */
        double t0, dt;
        nanosleep(&nap, 0);
        for (i = 0; i < T; ++i) { jobs[i].p = p; jobs[i].tid = i; jobs[i].calls = calls; jobs[i].objects = objects; jobs[i].bad = 0; }
        rio_op_device_round_trips(p, &b0, &r0);
        t0 = now_s();
        for (i = 0; i < T; ++i) pthread_create(&th[i], 0, worker, &jobs[i]);
        for (i = 0; i < T; ++i) { pthread_join(th[i], 0); bad += jobs[i].bad; }
        dt = now_s() - t0;
        rio_op_device_round_trips(p, &b1, &r1);
        if (r)
            printf("{\"label\": \"%s\", \"tracking\": %d, \"threads\": %d, \"calls\": %ld, \"calls_per_s\": %.4e, \"ns_per_call_per_thread\": %.1f, "
                   "\"device_round_trips\": %llu, \"wrong\": %d}\n", label, track, T, (long)T * calls, (double)T * calls / dt,
                   dt / calls * 1e9, (unsigned long long)(b1 - b0), bad);
        fflush(stdout);
    }
#ifndef NO_LOAD_TRACKING
    if (track) {  /* every lookup was counted: the fold says how many */
        uint64_t changed = 0, hits = 0;
        if (rio_op_fold_loads(p, 0, 1, 1, 0xFFFFFFFFu, &changed, &hits)) return 1;
        printf("{\"label\": \"%s\", \"hits_folded\": %llu, \"expected\": %lld}\n", label, (unsigned long long)hits,
               (long long)T * calls * (reps + 1));
        if (hits != (uint64_t)T * (uint64_t)calls * (uint64_t)(reps + 1)) bad++;
    }
#endif
    rio_op_release(p);
    return bad ? 3 : 0;
}
