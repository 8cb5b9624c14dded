/* preempt_round_host.c — the plain-C++ host steps of the preemption round (host.cpp: victim_uid_range behind ykhost_victim_range and
 * ykhost_preempt_round_by_keys, the argument checks of the round calls) on a MIRROR-ONLY handle (device -1), for a build of libykhost's
 * sources under AddressSanitizer + UBSan (tests/test_preempt_round_cpu.py). One node with four victims and a pod in no tier: every slice
 * of its order, buffers too short by one byte, slices past the end; then the round calls, which need a device and say so.
 * Exit code 0 and "preempt round host ok" = every call behaved. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ykhost.h"

static int failures = 0;
#define EXPECT(cond)                                                \
  do {                                                              \
    if (!(cond)) {                                                  \
      fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); \
      failures++;                                                   \
    }                                                               \
  } while (0)

#define POD(uid, prio, cpu)                                                                                                              \
  "{\"metadata\":{\"name\":\"" uid "\",\"uid\":\"" uid "\",\"namespace\":\"d\"},\"spec\":{\"priority\":" prio ",\"containers\":[{\"name\":\"c\"," \
  "\"resources\":{\"requests\":{\"cpu\":\"" cpu "\"}}}]}}"

static const char* kSnapshot =
    "{\"nodes\":["
    "{\"metadata\":{\"name\":\"n0\"},\"status\":{\"allocatable\":{\"cpu\":\"4\",\"memory\":\"1000\",\"pods\":\"30\"}},\"pods\":["
    POD("delta", "7", "100m") "," POD("bb", "0", "200m") "," POD("a", "0", "300m") "," POD("kept", "90", "100m") "," POD("charlie", "3", "400m") "]},"
    "{\"metadata\":{\"name\":\"n1\"},\"status\":{\"allocatable\":{\"cpu\":\"4\",\"memory\":\"1000\",\"pods\":\"30\"}},\"pods\":[]}],"
    "\"pods\":[" POD("ask", "50", "50m") "]}";

/* the slice as "a,b," beside what the call reported; the buffer is `len` bytes inside a poisoned frame */
static const char* range(ykhost_t* h, int node, int from, int count, int64_t len, int32_t* got, int64_t* needed) {
  static char flat[256];
  char* buf = (char*)malloc((size_t)len + 1);
  memset(buf, 0x55, (size_t)len + 1);
  flat[0] = 0;
  if (ykhost_victim_range(h, node, from, count, len ? buf : NULL, len, got, needed)) {
    free(buf);
    return "error";
  }
  const char* p = buf;
  int64_t used = 0;
  for (int i = 0; i < *got; ++i) {
    const size_t n = strnlen(p, (size_t)(len - used));
    if (used + (int64_t)n + 1 > len) break; /* this uid did not fit whole */
    strcat(flat, p), strcat(flat, ",");
    p += n + 1, used += (int64_t)n + 1;
  }
  if (buf[len] != 0x55) failures++, fprintf(stderr, "FAIL: wrote past the buffer\n");
  free(buf);
  return flat;
}

int main(void) {
  char err[256] = "";
  ykhost_t* h = ykhost_create(-1, err, sizeof err);
  if (!h) {
    fprintf(stderr, "ykhost_create(-1): %s\n", err);
    return 2;
  }
  int32_t got = -1;
  int64_t needed = -1;
  EXPECT(ykhost_load_snapshot(h, kSnapshot) == 0);
  EXPECT(ykhost_victim_range(h, 0, 0, 1, NULL, 0, &got, &needed) < 0 && got == 0); /* no tiers yet */
  const int32_t two[2] = {5, 10};
  EXPECT(ykhost_set_preemption_tiers(h, two, 2) == 0);
  /* order(n0) = a, bb (priority 0, by uid), charlie (3), delta (7); kept (90) is in no tier */
  EXPECT(strcmp(range(h, 0, 0, 4, 64, &got, &needed), "a,bb,charlie,delta,") == 0 && got == 4 && needed == 2 + 3 + 8 + 6);
  EXPECT(strcmp(range(h, 0, 1, 2, 64, &got, &needed), "bb,charlie,") == 0 && got == 2 && needed == 11);
  EXPECT(strcmp(range(h, 0, 3, 1, 64, &got, &needed), "delta,") == 0 && got == 1);
  EXPECT(strcmp(range(h, 0, 2, 0, 64, &got, &needed), "") == 0 && got == 0 && needed == 0);
  EXPECT(strcmp(range(h, 0, 3, 5, 64, &got, &needed), "delta,") == 0 && got == 1 && needed == 6); /* past the end: what there is */
  EXPECT(strcmp(range(h, 0, 4, 1, 64, &got, &needed), "") == 0 && got == 0);
  EXPECT(strcmp(range(h, 1, 0, 3, 64, &got, &needed), "") == 0 && got == 0 && needed == 0); /* a node without victims */
  /* buffers too short: whole uids only, the count and the need are the full ones, nothing is written past the end */
  EXPECT(strcmp(range(h, 0, 0, 4, 18, &got, &needed), "a,bb,charlie,") == 0 && got == 4 && needed == 19);
  EXPECT(strcmp(range(h, 0, 0, 4, 19, &got, &needed), "a,bb,charlie,delta,") == 0);
  EXPECT(strcmp(range(h, 0, 0, 4, 1, &got, &needed), "") == 0 && got == 4 && needed == 19);
  EXPECT(strcmp(range(h, 0, 0, 4, 0, &got, &needed), "") == 0 && got == 4 && needed == 19);
  EXPECT(ykhost_victim_range(h, 2, 0, 1, NULL, 0, &got, &needed) < 0 && ykhost_victim_range(h, -1, 0, 1, NULL, 0, &got, &needed) < 0);
  EXPECT(ykhost_victim_range(h, 0, -1, 1, NULL, 0, &got, &needed) < 0 && ykhost_victim_range(h, 0, 0, -1, NULL, 0, &got, &needed) < 0);
  EXPECT(ykhost_victim_range(h, 0, 0, 1, NULL, 0, NULL, &needed) < 0);
  EXPECT(ykhost_victim_range(h, 0, 0, 4, NULL, 0, &got, NULL) == 0 && got == 4);
  /* the slice follows the mirror: bb removed, the order closes up */
  EXPECT(ykhost_remove_pod(h, "bb") >= 0);
  EXPECT(strcmp(range(h, 0, 1, 2, 64, &got, &needed), "charlie,delta,") == 0 && got == 2);
  /* no device: the round calls refuse and leave their outputs alone */
  int64_t cells[16], summary[8], need2[2] = {7, 7};
  char names[64] = "x", uids[64] = "x";
  const char* keys[2] = {"ask", "ask"};
  const int32_t rows[1] = {0};
  memset(cells, 0x55, sizeof cells), memset(summary, 0x55, sizeof summary);
  EXPECT(ykhost_preempt_round(h, 1, rows, cells, summary) < 0);
  EXPECT(ykhost_preempt_round(h, -1, rows, cells, summary) < 0 && ykhost_preempt_round(h, 1, rows, cells, NULL) < 0);
  EXPECT(ykhost_preempt_round_by_keys(h, 2, keys, cells, summary, names, sizeof names, uids, sizeof uids, need2) < 0 && need2[0] == 0 && need2[1] == 0);
  EXPECT(ykhost_preempt_round_by_keys(h, 2, NULL, cells, summary, names, sizeof names, uids, sizeof uids, need2) < 0);
  EXPECT(ykhost_preempt_gang_by_key(h, "ask", 2, cells, summary, names, sizeof names, uids, sizeof uids, NULL) < 0);
  EXPECT(ykhost_preempt_gang_by_key(h, "ask", -1, cells, summary, names, sizeof names, uids, sizeof uids, need2) < 0);
  EXPECT(cells[0] == 0x5555555555555555ll && summary[7] == 0x5555555555555555ll && names[0] == 'x' && uids[0] == 'x');
  ykhost_destroy(h);
  if (failures) return 1;
  printf("preempt round host ok\n");
  return 0;
}
