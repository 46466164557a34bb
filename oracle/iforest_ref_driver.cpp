/*
 * iforest_ref_driver.cpp -- runs the reference's own include/isolation_forest.h on clouds read
 * from stdin (TEST INFRASTRUCTURE ONLY). This file is ours; the header is not in this
 * repository: `make -C oracle ref` finds it by -I in the reference tree and builds
 * _ref/iforest_ref_driver, which tests/test_oracle_iforest_ref.py compares with the
 * restatement (iforest_ref.h) bit for bit.
 *
 * stdin : records { int32 n, uint32 trees, uint32 seed, uint32 sample, float32 pts[n][3] }
 * stdout: per record { int32 ok, float64 scores[n] if ok }, ok = Build && GetAnomalyScores,
 *         the calls of Object_Map::IsolationForestDeleteOutliers (src/Object.cc:1202-1309).
 */
#include <array>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "isolation_forest.h"

int main() {
  int32_t n;
  uint32_t hdr[3];
  while (std::fread(&n, sizeof n, 1, stdin) == 1) {
    if (n < 0 || std::fread(hdr, sizeof hdr, 1, stdin) != 1) return 2;
    std::vector<std::array<float, 3>> data((size_t)n);
    if (n && std::fread(data.data(), sizeof data[0], (size_t)n, stdin) != (size_t)n) return 2;
    iforest::IsolationForest<float, 3> forest;
    std::vector<double> scores;
    int32_t ok = forest.Build(hdr[0], hdr[1], data, hdr[2]) && forest.GetAnomalyScores(data, scores) &&
                 scores.size() == (size_t)n;
    std::fwrite(&ok, sizeof ok, 1, stdout);
    if (ok && n) std::fwrite(scores.data(), sizeof(double), (size_t)n, stdout);
  }
  return std::fflush(stdout) == 0 ? 0 : 2;
}
