/* reclaim_table_host.c — the mirror's reclaim table (host.cpp: reclaim_column, reclaim_planes, ykhost_reclaim_table) and the ingest of
 * spec.priority / spec.preemptionPolicy / the allow-preemption annotation on a MIRROR-ONLY handle (device -1), for a build of libykhost's
 * sources under AddressSanitizer + UBSan (tests/test_preempt_reach_cpu.py). Two nodes, four residents in two tiers, one opted out, one
 * above the last bound; then a priority update, an assume, a forget, new bounds, a removal and a node removal, with the planes checked cell by cell after each.
 * Exit code 0 and "reclaim table ok" = every call behaved. */
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

static const char* kSnapshot =
    "{\"nodes\":["
    "{\"metadata\":{\"name\":\"n0\"},\"status\":{\"allocatable\":{\"cpu\":\"4\",\"memory\":\"1000\",\"pods\":\"10\"}},\"pods\":["
    "{\"metadata\":{\"name\":\"a\",\"uid\":\"a\",\"namespace\":\"d\"},\"spec\":{\"priority\":5,\"containers\":[{\"name\":\"c\",\"resources\":{\"requests\":{\"cpu\":\"100m\",\"memory\":\"7\"}},"
    "\"ports\":[{\"hostPort\":80,\"containerPort\":80}]}]}},"
    "{\"metadata\":{\"name\":\"b\",\"uid\":\"b\",\"namespace\":\"d\"},\"spec\":{\"containers\":[{\"name\":\"c\",\"resources\":{\"requests\":{\"cpu\":\"200m\"}}}]}},"
    "{\"metadata\":{\"name\":\"c\",\"uid\":\"c\",\"namespace\":\"d\",\"annotations\":{\"yunikorn.apache.org/allow-preemption\":\"false\"}},"
    "\"spec\":{\"priority\":-3,\"containers\":[{\"name\":\"c\",\"resources\":{\"requests\":{\"cpu\":\"400m\"}}}]}}]},"
    "{\"metadata\":{\"name\":\"n1\"},\"status\":{\"allocatable\":{\"cpu\":\"4\",\"memory\":\"1000\",\"pods\":\"10\"}},\"pods\":["
    "{\"metadata\":{\"name\":\"e\",\"uid\":\"e\",\"namespace\":\"d\"},\"spec\":{\"priority\":50,\"containers\":[{\"name\":\"c\",\"resources\":{\"requests\":{\"cpu\":\"800m\"}}}]}}]}],"
    "\"pods\":[{\"metadata\":{\"name\":\"ask\",\"uid\":\"ask\",\"namespace\":\"d\"},\"spec\":{\"priority\":9,\"preemptionPolicy\":\"Never\",\"containers\":[{\"name\":\"c\","
    "\"resources\":{\"requests\":{\"cpu\":\"50m\"}},\"ports\":[{\"hostPort\":80,\"containerPort\":80}]}]}}]}";

/* planes of at most 8 tiers x 8 dimensions x 4 port words x 2 nodes */
static int64_t req[8 * 8 * 2];
static int32_t pods[8 * 2];
static uint64_t ports[8 * 4 * 2];
static int32_t dims[4];

static int table(ykhost_t* h) {
  memset(req, 0x55, sizeof req), memset(pods, 0x55, sizeof pods), memset(ports, 0x55, sizeof ports);
  int rc = ykhost_reclaim_table(h, dims, NULL, NULL, NULL);
  if (rc) return rc;
  if (dims[0] > 8 || dims[1] > 8 || dims[2] > 4 || dims[3] > 2) return -99;
  return ykhost_reclaim_table(h, dims, req, pods, ports);
}
#define REQ(t, r, n) req[((t) * dims[1] + (r)) * dims[3] + (n)]
#define PODS(t, n) pods[(t) * dims[3] + (n)]
#define PORT0(t, n) ports[((t) * dims[2]) * dims[3] + (n)]

int main(void) {
  char err[256] = "";
  ykhost_t* h = ykhost_create(-1, err, sizeof err);
  if (!h) {
    fprintf(stderr, "ykhost_create(-1): %s\n", err);
    return 2;
  }
  EXPECT(ykhost_load_snapshot(h, kSnapshot) == 0);
  EXPECT(ykhost_reclaim_table(h, dims, NULL, NULL, NULL) < 0); /* no tiers yet */
  EXPECT(ykhost_reclaim_table(h, NULL, NULL, NULL, NULL) < 0);
  const int32_t bad[2] = {10, 10}, two[2] = {1, 10}, three[3] = {-3, 6, 60};
  EXPECT(ykhost_set_preemption_tiers(h, bad, 2) < 0);
  EXPECT(ykhost_set_preemption_tiers(h, two, 9) < 0);
  EXPECT(ykhost_set_preemption_tiers(h, two, 2) == 0);
  /* tier 0: priority < 1: b (missing = 0); c is below too but opted out. tier 1: a (5). e (50) is in no tier. */
  EXPECT(table(h) == 0);
  EXPECT(dims[0] == 2 && dims[1] == 3 && dims[2] == 1 && dims[3] == 2);
  EXPECT(PODS(0, 0) == 1 && PODS(1, 0) == 1 && PODS(0, 1) == 0 && PODS(1, 1) == 0);
  EXPECT(REQ(0, 0, 0) == 200 && REQ(1, 0, 0) == 100 && REQ(1, 1, 0) == 7 && REQ(0, 1, 0) == 0 && REQ(0, 0, 1) == 0 && REQ(1, 0, 1) == 0);
  EXPECT(PORT0(0, 0) == 1 && PORT0(1, 0) == 0 && PORT0(0, 1) == 0); /* a holds the one dictionary port until tier 1 goes */
  /* a priority update moves a into tier 0 */
  EXPECT(ykhost_update_pod(h, "{\"metadata\":{\"name\":\"a\",\"uid\":\"a\",\"namespace\":\"d\"},\"spec\":{\"nodeName\":\"n0\",\"priority\":0,\"containers\":[{\"name\":\"c\","
                              "\"resources\":{\"requests\":{\"cpu\":\"100m\",\"memory\":\"7\"}},\"ports\":[{\"hostPort\":80,\"containerPort\":80}]}]},"
                              "\"status\":{\"phase\":\"Running\"}}") == 1);
  EXPECT(table(h) == 0);
  EXPECT(PODS(0, 0) == 2 && PODS(1, 0) == 0 && REQ(0, 0, 0) == 300 && REQ(0, 1, 0) == 7 && REQ(1, 0, 0) == 0 && PORT0(0, 0) == 0 && PORT0(1, 0) == 0);
  /* the ask (priority 9) assumed on n1 is a tier-1 pod there; forgotten it stays */
  EXPECT(ykhost_assume_pod(h, "ask", "n1") == 0);
  EXPECT(table(h) == 0);
  EXPECT(PODS(1, 1) == 1 && REQ(1, 0, 1) == 50 && PODS(0, 1) == 0 && PORT0(0, 1) == 1 && PORT0(1, 1) == 0);
  EXPECT(ykhost_forget_pod(h, "ask") >= 0);
  EXPECT(table(h) == 0 && PODS(1, 1) == 1);
  /* new bounds: tier 0 < -3 nobody; tier 1 < 6: a, b (c opted out); tier 2 < 60: e and the ask */
  EXPECT(ykhost_set_preemption_tiers(h, three, 3) == 0);
  EXPECT(table(h) == 0);
  EXPECT(dims[0] == 3 && PODS(0, 0) == 0 && PODS(1, 0) == 2 && PODS(2, 0) == 0 && PODS(2, 1) == 2 && REQ(2, 0, 1) == 850 && REQ(1, 0, 0) == 300);
  EXPECT(PORT0(0, 0) == 1 && PORT0(1, 0) == 0 && PORT0(2, 0) == 0 && PORT0(1, 1) == 1 && PORT0(2, 1) == 0);
  EXPECT(ykhost_remove_pod(h, "ask") >= 0);
  EXPECT(table(h) == 0 && PODS(2, 1) == 1 && REQ(2, 0, 1) == 800);
  /* a node removal shifts the columns */
  EXPECT(ykhost_remove_node(h, "n0") >= 0);
  EXPECT(table(h) == 0);
  EXPECT(dims[3] == 1 && PODS(2, 0) == 1 && REQ(2, 0, 0) == 800 && PODS(1, 0) == 0);
  /* no device: the reach calls refuse, with their cells as promised */
  int64_t cells[16];
  int32_t levels[2];
  char name[64] = "x";
  EXPECT(ykhost_preempt_reach(h, 0, NULL, cells) < 0);
  EXPECT(ykhost_preempt_reach_nodes(h, 0, levels) < 0);
  EXPECT(ykhost_preempt_reach_by_key(h, "no-such-pod", cells, name, sizeof name) == YKHOST_E_POD_NOT_FOUND && cells[13] == -1 && name[0] == 0);
  EXPECT(ykhost_preempt_reach_by_key(h, "e", cells, name, sizeof name) == YKHOST_E_NOT_AN_ASK);
  EXPECT(ykhost_set_preemption_tiers(h, NULL, 0) == 0);
  EXPECT(ykhost_reclaim_table(h, dims, NULL, NULL, NULL) < 0);
  ykhost_destroy(h);
  if (failures) return 1;
  printf("reclaim table ok\n");
  return 0;
}
