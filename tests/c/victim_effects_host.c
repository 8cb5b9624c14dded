/* victim_effects_host.c — the plain-C++ host steps behind the victim-effects plane (host.cpp: victim_effects_refresh behind
 * ykhost_victim_effects, the argument checks of the live round calls) on a MIRROR-ONLY handle (device -1), for a build of libykhost's
 * sources under AddressSanitizer + UBSan (tests/test_preempt_round_live_cpu.py). One node with four victims — three of them match the
 * ask's spread selector — and a matching pod in no tier: the plane's columns and prefix sums, its patching when a pod leaves and when
 * one arrives, its re-derivation when a class gains its first contributing victim; then the live round calls, which need a device and
 * say so. Exit code 0 and "victim effects host ok" = every call behaved. */
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

#define POD(uid, prio, app)                                                                                                            \
  "{\"metadata\":{\"name\":\"" uid "\",\"uid\":\"" uid "\",\"namespace\":\"d\",\"labels\":{\"app\":\"" app "\"}},\"spec\":{\"priority\":" prio \
  ",\"containers\":[{\"name\":\"c\",\"resources\":{\"requests\":{\"cpu\":\"100m\"}}}]}}"
#define SPREAD(app) \
  "{\"maxSkew\":1,\"topologyKey\":\"zone\",\"whenUnsatisfiable\":\"DoNotSchedule\",\"labelSelector\":{\"matchLabels\":{\"app\":\"" app "\"}}}"
#define ASK(uid, app)                                                                                                                      \
  "{\"metadata\":{\"name\":\"" uid "\",\"uid\":\"" uid "\",\"namespace\":\"d\",\"labels\":{\"app\":\"x\"}},\"spec\":{\"priority\":50,\"containers\":[{" \
  "\"name\":\"c\",\"resources\":{\"requests\":{\"cpu\":\"50m\"}}}],\"topologySpreadConstraints\":[" SPREAD(app) "]}}"
#define NODE(name, pods)                                                                                                               \
  "{\"metadata\":{\"name\":\"" name "\",\"labels\":{\"zone\":\"z\"}},\"status\":{\"allocatable\":{\"cpu\":\"4\",\"memory\":\"1000\",\"pods\":\"30\"}}," \
  "\"pods\":[" pods "]}"

static const char* kSnapshot =
    "{\"nodes\":[" NODE("n0", POD("delta", "7", "web") "," POD("bb", "0", "web") "," POD("a", "0", "web") "," POD("kept", "90", "web") ","
                                                                                                                  POD("charlie", "3", "res"))
    "," NODE("n1", "") "],\"pods\":[" ASK("ask-web", "web") "," ASK("ask-db", "db") "]}";

/* the plane copied out into exactly-sized blocks: dims = { KS, KA, P, derived, patches } */
static int plane(ykhost_t* h, int32_t* dims, int32_t** col, int32_t** cum) {
  *col = *cum = NULL;
  if (ykhost_victim_effects(h, dims, NULL, NULL)) return -1;
  *col = (int32_t*)malloc(sizeof(int32_t) * (size_t)(dims[0] + 1));
  *cum = (int32_t*)malloc(sizeof(int32_t) * ((size_t)dims[1] * (size_t)dims[2] + 1));
  (*col)[dims[0]] = 0x55555555;
  (*cum)[(size_t)dims[1] * (size_t)dims[2]] = 0x55555555;
  const int rc = ykhost_victim_effects(h, dims, *col, *cum);
  if ((*col)[dims[0]] != 0x55555555 || (*cum)[(size_t)dims[1] * (size_t)dims[2]] != 0x55555555) failures++, fprintf(stderr, "FAIL: wrote past a buffer\n");
  return rc;
}

int main(void) {
  char err[256] = "";
  ykhost_t* h = ykhost_create(-1, err, sizeof err);
  if (!h) {
    fprintf(stderr, "ykhost_create(-1): %s\n", err);
    return 2;
  }
  int32_t dims[5] = {-1, -1, -1, -1, -1}, *col = NULL, *cum = NULL;
  EXPECT(ykhost_load_snapshot(h, kSnapshot) == 0);
  EXPECT(ykhost_victim_effects(h, dims, NULL, NULL) < 0); /* no tiers yet */
  EXPECT(ykhost_victim_effects(h, NULL, NULL, NULL) < 0);
  const int32_t two[2] = {5, 10};
  EXPECT(ykhost_set_preemption_tiers(h, two, 2) == 0);
  int32_t vdims[5];
  EXPECT(ykhost_victim_table(h, vdims, NULL, NULL, NULL, NULL, NULL) == 0);
  /* order(n0) = a, bb (priority 0, by uid), charlie (3), delta (7); kept (90) is in no tier. Two selector classes (web, db); only web
   * has a contributing victim: one column. Segment of n0: rows 0..9 (4 + 2 + 4), n1: 4 rows. */
  EXPECT(plane(h, dims, &col, &cum) == 0);
  EXPECT(dims[0] == 2 && dims[1] == 1 && dims[2] == vdims[4] && dims[2] == 14 && dims[3] == 1 && dims[4] == 0);
  int web = col[0] >= 0 ? 0 : 1;
  EXPECT(col[web] == 0 && col[1 - web] == -1);
  EXPECT(cum[0] == 1 && cum[1] == 2 && cum[2] == 2 && cum[3] == 3);
  free(col), free(cum);
  /* bb leaves: the segment is patched, nothing is derived anew */
  EXPECT(ykhost_remove_pod(h, "bb") >= 0);
  EXPECT(plane(h, dims, &col, &cum) == 0);
  EXPECT(dims[1] == 1 && dims[3] == 1 && dims[4] == 1 && cum[0] == 1 && cum[1] == 1 && cum[2] == 2);
  free(col), free(cum);
  /* a db pod arrives on n1 as a victim: the class gains its first contributing victim — a second column, the plane derived anew */
  EXPECT(ykhost_update_pod(h, "{\"metadata\":{\"name\":\"db0\",\"uid\":\"db0\",\"namespace\":\"d\",\"labels\":{\"app\":\"db\"}},\"spec\":{\"nodeName\":\"n1\","
                              "\"priority\":1,\"containers\":[{\"name\":\"c\",\"resources\":{\"requests\":{\"cpu\":\"100m\"}}}]},\"status\":{\"phase\":\"Running\"}}") >= 0);
  EXPECT(plane(h, dims, &col, &cum) == 0);
  EXPECT(dims[0] == 2 && dims[1] == 2 && dims[3] == 2 && col[0] >= 0 && col[1] >= 0 && col[0] != col[1]);
  if (dims[1] == 2) {
    const int32_t P = dims[2], n1 = 10; /* n1's segment begins behind n0's ten rows */
    EXPECT(cum[(size_t)col[1 - web] * (size_t)P + n1] == 1 && cum[(size_t)col[web] * (size_t)P + n1] == 0);
    EXPECT(cum[(size_t)col[web] * (size_t)P + 2] == 2 && cum[(size_t)col[1 - web] * (size_t)P + 2] == 0);
  }
  free(col), free(cum);
  /* no device: the live round calls refuse and leave their outputs alone */
  int64_t cells[16], summary[8], need2[2] = {7, 7};
  int32_t counts[4] = {7, 7, 7, 7}, minima[4] = {7, 7, 7, 7};
  char names[64] = "x", uids[64] = "x";
  const char* keys[2] = {"ask-web", "ask-web"};
  const int32_t rows[1] = {0};
  memset(cells, 0x55, sizeof cells), memset(summary, 0x55, sizeof summary);
  EXPECT(ykhost_preempt_round_live(h, 1, rows, cells, summary, counts, 4, minima, 4, need2) < 0 && need2[0] == 0 && need2[1] == 0);
  EXPECT(ykhost_preempt_round_live(h, -1, rows, cells, summary, NULL, 0, NULL, 0, NULL) < 0);
  EXPECT(ykhost_preempt_round_live(h, 1, rows, cells, NULL, NULL, 0, NULL, 0, NULL) < 0);
  EXPECT(ykhost_preempt_round_live(h, 1, rows, cells, summary, counts, -1, minima, 4, NULL) < 0);
  need2[0] = need2[1] = 7;
  EXPECT(ykhost_preempt_round_live_by_keys(h, 2, keys, cells, summary, names, sizeof names, uids, sizeof uids, need2) < 0 && need2[0] == 0);
  EXPECT(ykhost_preempt_round_live_by_keys(h, 2, NULL, cells, summary, names, sizeof names, uids, sizeof uids, need2) < 0);
  EXPECT(ykhost_preempt_gang_live_by_key(h, "ask-web", 2, cells, summary, names, sizeof names, uids, sizeof uids, NULL) < 0);
  EXPECT(ykhost_preempt_gang_live_by_key(h, "ask-web", -1, cells, summary, names, sizeof names, uids, sizeof uids, need2) < 0);
  EXPECT(cells[0] == 0x5555555555555555ll && summary[7] == 0x5555555555555555ll && names[0] == 'x' && uids[0] == 'x' && counts[0] == 7 && minima[3] == 7);
  ykhost_destroy(h);
  if (failures) return 1;
  printf("victim effects host ok\n");
  return 0;
}
