// packed_rows_demo.cpp -- PCA::addClouds against the rows of the batch extract added one by one
// (test_gpu_packed_rows_facade.py runs it):
//   packed_rows_demo <leaf> <subdiv> <cloud.bin>...
// Clouds are n x 4 floats (x y z rgb).  Variant 117 plain and variant 981 with the 24 rotations: the
// batch form of extractC3HLACSignature over all clouds, every row with a non-zero value (what
// writeFeature keeps) into PCA::addData / addDataRotated24, solve; then PCA::addClouds over the same
// clouds, solve.  Prints, as JSON, per variant the rows added on either route and the largest
// difference of the variances relative to the largest variance.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <vector>

#include "c3hlac_host.h"

using namespace c3hlac;

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  try {
    const float leaf = (float)atof(argv[1]);
    const int subdiv = atoi(argv[2]);
    std::vector<std::vector<PointXYZRGB> > clouds;
    for (int i = 3; i < argc; ++i) {
      std::ifstream in(argv[i], std::ios::binary);
      std::vector<PointXYZRGB> cloud;
      PointXYZRGB p;
      while (in.read(reinterpret_cast<char*>(&p), sizeof(p))) cloud.push_back(p);
      clouds.push_back(cloud);
    }
    Context ctx(0);
    printf("{");
    for (int variant : {117, 981}) {
      const bool rotated = variant == 981;
      std::vector<std::vector<std::vector<float> > > rows;
      if (variant == 981) extractC3HLACSignature981(ctx, clouds, rows, 147, 146, 148, leaf, subdiv);
      else extractC3HLACSignature117(ctx, clouds, rows, 147, 146, 148, leaf, subdiv);
      PCA one(false), all(false);
      long kept = 0;
      for (const auto& cloud : rows)
        for (const auto& row : cloud) {
          if (std::all_of(row.begin(), row.end(), [](float v) { return v == 0.0f; })) continue;
          if (rotated) one.addDataRotated24(row);
          else one.addData(row);
          ++kept;
        }
      one.solve();
      const long added = (long)all.addClouds(ctx, clouds, variant, 147, 146, 148, leaf, subdiv, Vector3i(), C3H_COLOR_C3_DOUBLE, rotated);
      all.solve();
      double worst = 0;
      const std::vector<float>&a = one.getVariance(), &b = all.getVariance();
      for (size_t i = 0; i < a.size() && i < b.size(); ++i) worst = std::max(worst, std::fabs((double)a[i] - (double)b[i]));
      printf("%s\"%d\": {\"kept\": %ld, \"added\": %ld, \"dim\": [%zu, %zu], \"variance_diff\": %.3e}", variant == 117 ? "" : ", ",
             variant, kept, added, a.size(), b.size(), a.empty() || a[0] == 0 ? -1.0 : worst / a[0]);
    }
    printf("}\n");
    return 0;
  } catch (const std::exception& e) {
    fprintf(stderr, "packed_rows_demo: %s\n", e.what());
    return 1;
  }
}
