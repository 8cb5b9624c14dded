/* victim_table_host.c — the mirror's victim table (host.cpp: victim_order, victim_segment, victims_refresh, ykhost_victim_table,
 * ykhost_victim_list) on a MIRROR-ONLY handle (device -1), for a build of libykhost's sources under AddressSanitizer + UBSan
 * (tests/test_preempt_victims_cpu.py). Two nodes, five residents, one opted out, one above the last bound; then a priority update, an
 * assume, growth past a segment's capacity, a removal, new bounds and a node removal, with the planes checked cell by cell after each.
 * Exit code 0 and "victim table ok" = every call behaved. */
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

#define POD(uid, prio, cpu, extra)                                                                                                        \
  "{\"metadata\":{\"name\":\"" uid "\",\"uid\":\"" uid "\",\"namespace\":\"d\"" extra "},\"spec\":{\"priority\":" prio ",\"containers\":[{\"name\":\"c\"," \
  "\"resources\":{\"requests\":{\"cpu\":\"" cpu "\"}}}]}}"
#define RUNNING(uid, prio, cpu, node)                                                                                                    \
  "{\"metadata\":{\"name\":\"" uid "\",\"uid\":\"" uid "\",\"namespace\":\"d\"},\"spec\":{\"nodeName\":\"" node "\",\"priority\":" prio ",\"containers\":[{\"name\":\"c\"," \
  "\"resources\":{\"requests\":{\"cpu\":\"" cpu "\"}}}]},\"status\":{\"phase\":\"Running\"}}"

static const char* kSnapshot =
    "{\"nodes\":["
    "{\"metadata\":{\"name\":\"n0\"},\"status\":{\"allocatable\":{\"cpu\":\"4\",\"memory\":\"1000\",\"pods\":\"30\"}},\"pods\":["
    "{\"metadata\":{\"name\":\"a\",\"uid\":\"a\",\"namespace\":\"d\"},\"spec\":{\"priority\":5,\"containers\":[{\"name\":\"c\",\"resources\":{\"requests\":{\"cpu\":\"100m\",\"memory\":\"7\"}},"
    "\"ports\":[{\"hostPort\":80,\"containerPort\":80}]}]}},"
    POD("z", "0", "200m", "") ","
    POD("b", "0", "300m", "") ","
    POD("c", "-3", "400m", ",\"annotations\":{\"yunikorn.apache.org/allow-preemption\":\"false\"}") "]},"
    "{\"metadata\":{\"name\":\"n1\"},\"status\":{\"allocatable\":{\"cpu\":\"4\",\"memory\":\"1000\",\"pods\":\"30\"}},\"pods\":["
    POD("e", "50", "800m", "") "]}],"
    "\"pods\":[{\"metadata\":{\"name\":\"ask\",\"uid\":\"ask\",\"namespace\":\"d\"},\"spec\":{\"priority\":9,\"containers\":[{\"name\":\"c\","
    "\"resources\":{\"requests\":{\"cpu\":\"50m\"}},\"ports\":[{\"hostPort\":80,\"containerPort\":80}]}]}}]}";

/* planes of at most 8 tiers x 8 dimensions x 4 port words x 2 nodes x 64 rows */
static int32_t base[2], cap[2], tier_end[8 * 2];
static int64_t cum[8 * 64];
static uint64_t ports[4 * 64];
static int32_t dims[5];
static int64_t stats[2];

static int table(ykhost_t* h) {
  memset(base, 0x55, sizeof base), memset(cap, 0x55, sizeof cap), memset(tier_end, 0x55, sizeof tier_end);
  memset(cum, 0x55, sizeof cum), memset(ports, 0x55, sizeof ports);
  int rc = ykhost_victim_table(h, dims, NULL, NULL, NULL, NULL, NULL);
  if (rc) return rc;
  if (dims[0] > 8 || dims[1] > 8 || dims[2] > 4 || dims[3] > 2 || dims[4] > 64) return -99;
  rc = ykhost_victim_table(h, dims, base, cap, tier_end, cum, ports);
  if (rc) return rc;
  return ykhost_victim_stats(h, stats);
}
#define END(t, n) tier_end[(t) * dims[3] + (n)]
#define CUM(r, n, i) cum[(r) * dims[4] + base[n] + (i)]
#define PORT0(n, i) ports[base[n] + (i)]

/* the NUL-separated list as "a,b," */
static const char* list(ykhost_t* h, int node, int limit, int32_t* count) {
  static char buf[256], flat[256];
  memset(buf, 0x55, sizeof buf);
  flat[0] = 0;
  if (ykhost_victim_list(h, node, limit, buf, sizeof buf, count)) return "error";
  const char* p = buf;
  for (int i = 0; i < *count; ++i) {
    strcat(flat, p), strcat(flat, ",");
    p += strlen(p) + 1;
  }
  return flat;
}

int main(void) {
  char err[256] = "";
  ykhost_t* h = ykhost_create(-1, err, sizeof err);
  if (!h) {
    fprintf(stderr, "ykhost_create(-1): %s\n", err);
    return 2;
  }
  int32_t count = -1;
  EXPECT(ykhost_load_snapshot(h, kSnapshot) == 0);
  EXPECT(ykhost_victim_table(h, dims, NULL, NULL, NULL, NULL, NULL) < 0); /* no tiers yet */
  EXPECT(ykhost_victim_list(h, 0, 0, NULL, 0, &count) < 0 && count == 0);
  const int32_t two[2] = {1, 10}, three[3] = {-3, 6, 60};
  EXPECT(ykhost_set_preemption_tiers(h, two, 2) == 0);
  EXPECT(ykhost_victim_stats(h, stats) == 0 && stats[0] == 0 && stats[1] == 0); /* nothing derived before the first victims call */
  /* tier 0 (priority < 1): b and z at priority 0, by uid; c is below but opted out. tier 1: a (5). e (50) is in no tier. */
  EXPECT(table(h) == 0);
  EXPECT(dims[0] == 2 && dims[1] == 3 && dims[2] == 1 && dims[3] == 2);
  EXPECT(stats[0] == 1 && stats[1] == 0);
  EXPECT(cap[0] == 3 + 1 + 4 && cap[1] == 4 && base[0] == 0 && base[1] == cap[0] && dims[4] == cap[0] + cap[1]);
  EXPECT(END(0, 0) == 2 && END(1, 0) == 3 && END(0, 1) == 0 && END(1, 1) == 0);
  EXPECT(CUM(0, 0, 0) == 300 && CUM(0, 0, 1) == 500 && CUM(0, 0, 2) == 600 && CUM(1, 0, 1) == 0 && CUM(1, 0, 2) == 7);
  EXPECT(PORT0(0, 0) == 1 && PORT0(0, 1) == 1 && PORT0(0, 2) == 0); /* a, the last of the order, holds the one dictionary port */
  EXPECT(strcmp(list(h, 0, 2, &count), "b,z,a,") == 0 && count == 3);
  EXPECT(strcmp(list(h, 0, 1, &count), "b,z,") == 0 && count == 2);
  EXPECT(strcmp(list(h, 0, 0, &count), "") == 0 && count == 0);
  EXPECT(strcmp(list(h, 1, 2, &count), "") == 0 && count == 0);
  /* a buffer that takes one uid whole: the count is still the full number */
  char tiny[3] = {0x55, 0x55, 0x55};
  EXPECT(ykhost_victim_list(h, 0, 2, tiny, 3, &count) == 0 && count == 3 && strcmp(tiny, "b") == 0 && tiny[2] == 0x55);
  EXPECT(ykhost_victim_list(h, 2, 2, tiny, 3, &count) < 0 && ykhost_victim_list(h, 0, 3, tiny, 3, &count) < 0);
  /* a priority update moves a in front of b and z: ONE segment patched */
  EXPECT(ykhost_update_pod(h, "{\"metadata\":{\"name\":\"a\",\"uid\":\"a\",\"namespace\":\"d\"},\"spec\":{\"nodeName\":\"n0\",\"priority\":-1,\"containers\":[{\"name\":\"c\","
                              "\"resources\":{\"requests\":{\"cpu\":\"100m\",\"memory\":\"7\"}},\"ports\":[{\"hostPort\":80,\"containerPort\":80}]}]},"
                              "\"status\":{\"phase\":\"Running\"}}") == 1);
  EXPECT(table(h) == 0 && stats[0] == 1 && stats[1] == 1);
  EXPECT(END(0, 0) == 3 && END(1, 0) == 3 && CUM(0, 0, 0) == 100 && CUM(1, 0, 0) == 7 && CUM(0, 0, 2) == 600 && PORT0(0, 0) == 0 && PORT0(0, 2) == 0);
  EXPECT(strcmp(list(h, 0, 1, &count), "a,b,z,") == 0);
  /* the ask (priority 9) assumed on n1 is a tier-1 victim there, holding the port */
  EXPECT(ykhost_assume_pod(h, "ask", "n1") == 0);
  EXPECT(table(h) == 0 && stats[0] == 1 && stats[1] == 2);
  EXPECT(END(0, 1) == 0 && END(1, 1) == 1 && CUM(0, 1, 0) == 50 && PORT0(1, 0) == 0 && strcmp(list(h, 1, 2, &count), "ask,") == 0);
  /* four more on n1: five victims pass its capacity of four — the whole table is derived anew, with room again */
  EXPECT(ykhost_update_pod(h, RUNNING("g0", "1", "10m", "n1")) >= 0 && ykhost_update_pod(h, RUNNING("g1", "1", "10m", "n1")) >= 0);
  EXPECT(ykhost_update_pod(h, RUNNING("g2", "0", "10m", "n1")) >= 0);
  EXPECT(table(h) == 0 && stats[0] == 1 && END(1, 1) == 4 && END(0, 1) == 1 && CUM(0, 1, 0) == 10 && CUM(0, 1, 3) == 80);
  EXPECT(ykhost_update_pod(h, RUNNING("g3", "2", "10m", "n1")) >= 0);
  EXPECT(table(h) == 0 && stats[0] == 2 && cap[1] == 5 + 2 + 4 && END(1, 1) == 5 && CUM(0, 1, 4) == 90);
  EXPECT(strcmp(list(h, 1, 2, &count), "g2,g0,g1,g3,ask,") == 0 && count == 5);
  /* a removal: patched in place, the capacity stays */
  const int64_t patches = stats[1];
  EXPECT(ykhost_remove_pod(h, "g0") >= 0);
  EXPECT(table(h) == 0 && stats[0] == 2 && stats[1] == patches + 1 && cap[1] == 11 && END(1, 1) == 4 && CUM(0, 1, 3) == 80);
  /* new bounds: tier 0 < -3 nobody; tier 1 < 6: a, b, z and g1, g2, g3; tier 2 < 60: e and the ask */
  EXPECT(ykhost_set_preemption_tiers(h, three, 3) == 0);
  EXPECT(table(h) == 0 && stats[0] == 3 && dims[0] == 3);
  EXPECT(END(0, 0) == 0 && END(1, 0) == 3 && END(2, 0) == 3 && END(0, 1) == 0 && END(1, 1) == 3 && END(2, 1) == 5);
  EXPECT(strcmp(list(h, 1, 3, &count), "g2,g1,g3,ask,e,") == 0 && CUM(0, 1, 4) == 880);
  /* a node removal: another node count, the whole table again */
  EXPECT(ykhost_remove_node(h, "n0") >= 0);
  EXPECT(table(h) == 0 && stats[0] == 4 && dims[3] == 1 && base[0] == 0 && END(2, 0) == 5);
  /* no device: the victims calls refuse, with their cells as promised */
  int64_t cells[16];
  int32_t needs[2];
  char name[64] = "x", uids[64] = "x";
  EXPECT(ykhost_preempt_victims(h, 0, NULL, cells) < 0);
  EXPECT(ykhost_preempt_victims_nodes(h, 0, needs) < 0);
  EXPECT(ykhost_preempt_victims_by_key(h, "no-such-pod", cells, name, sizeof name, uids, sizeof uids) == YKHOST_E_POD_NOT_FOUND && cells[6] == -1 &&
         name[0] == 0 && uids[0] == 0);
  EXPECT(ykhost_preempt_victims_by_key(h, "e", cells, name, sizeof name, uids, sizeof uids) == YKHOST_E_NOT_AN_ASK);
  EXPECT(ykhost_set_preemption_tiers(h, NULL, 0) == 0);
  EXPECT(ykhost_victim_table(h, dims, NULL, NULL, NULL, NULL, NULL) < 0);
  ykhost_destroy(h);
  if (failures) return 1;
  printf("victim table ok\n");
  return 0;
}
