// c3_rows_demo.cpp -- the batch form of extractC3HLACSignature981/117 against the single-cloud one
// (test_gpu_c3_rows_facade.py runs it):
//   c3_rows_demo <leaf> <subdiv> <cloud.bin>...
// Clouds are n x 4 floats (x y z rgb).  For both variants: getVoxelGrid + extractC3HLACSignature of
// every cloud in turn, then the batch function over all clouds; rows and counts are compared as
// bytes.  Prints, as JSON, per variant the rows per cloud, the number of rows with a non-zero value
// and the number of differing clouds.
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
    for (int variant : {981, 117}) {
      std::vector<std::vector<std::vector<float> > > single(clouds.size()), batch;
      std::vector<Vector3i> sb1(clouds.size());
      for (size_t i = 0; i < clouds.size(); ++i) {
        VoxelGrid grid(ctx);
        std::vector<PointXYZRGB> down;
        getVoxelGrid(grid, clouds[i], down, leaf);
        sb1[i] = variant == 981 ? extractC3HLACSignature981(grid, single[i], 147, 146, 148, leaf, subdiv)
                                : extractC3HLACSignature117(grid, single[i], 147, 146, 148, leaf, subdiv);
      }
      std::vector<c3h_frame_info> info;
      const std::vector<Vector3i> sb = variant == 981
          ? extractC3HLACSignature981(ctx, clouds, batch, 147, 146, 148, leaf, subdiv, 0, 0, 0, C3H_COLOR_C3_DOUBLE,
                                      std::numeric_limits<float>::infinity(), &info)
          : extractC3HLACSignature117(ctx, clouds, batch, 147, 146, 148, leaf, subdiv, 0, 0, 0, C3H_COLOR_C3_DOUBLE,
                                      std::numeric_limits<float>::infinity(), &info);
      int differ = 0;
      long nonzero = 0;
      printf("%s\"%d\": {\"rows\": [", variant == 981 ? "" : ", ", variant);
      for (size_t i = 0; i < clouds.size(); ++i) {
        bool same = batch[i].size() == single[i].size() && sb[i][0] == sb1[i][0] && sb[i][1] == sb1[i][1] &&
                    sb[i][2] == sb1[i][2] && info[i].status == 0;
        for (size_t h = 0; same && h < batch[i].size(); ++h) {
          same = batch[i][h].size() == (size_t)variant && single[i][h].size() == (size_t)variant &&
                 memcmp(batch[i][h].data(), single[i][h].data(), (size_t)variant * sizeof(float)) == 0;
          bool nz = false;
          for (float v : batch[i][h]) nz = nz || v != 0.0f;
          nonzero += nz;
        }
        differ += !same;
        printf(i ? ", %zu" : "%zu", batch[i].size());
      }
      printf("], \"nonzero\": %ld, \"differ\": %d}", nonzero, differ);
    }
    printf("}\n");
    return 0;
  } catch (const std::exception& e) {
    fprintf(stderr, "c3_rows_demo: %s\n", e.what());
    return 1;
  }
}
