/*
 * depth_register_demo.cpp — a raw 16-bit sensor depth frame into the engine: prep::DepthMap aligns it to the colour camera
 * on the device (the step the reference's grabber leaves to the vendor SDK, k4a_grabber.h:339-340), Cloud::fromDepth
 * back-projects the aligned image.  Prints the counters of the registration and the scene cloud's size.
 *
 *   usage: depth_register_demo depth.u16 scale calib.f64
 *          depth.u16  raw little-endian uint16, depth_rows x depth_cols, z = d * scale metres
 *          calib.f64  raw little-endian doubles: depth_rows depth_cols, the 13 camera values fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6
 *                     max_r of the depth camera, color_rows color_cols, the 13 of the colour camera, R (9, row-major), t (3)
 *   build: g++ -std=c++11 -Iinclude examples/depth_register_demo.cpp -Lyolo_ppf_pose_estimation_amd/csrc -lppf_hip
 */
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "ppf_cloud_stages.hpp"

using namespace std;
using namespace ppfhip;

template <class T>
static void read_raw(const char* path, vector<T>& v, size_t count) {
  ifstream f(path, ios::binary);
  if (!f.read(reinterpret_cast<char*>(&v[0]), (streamsize)(count * sizeof(T))))
    throw ppf_match_3d::Error(PPF_ERR_IO, string("cannot read ") + path);
}

static ppf_camera camera_of(const double* v) {
  ppf_camera c = prep::DepthMap::pinhole(v[0], v[1], v[2], v[3]);
  c.k1 = v[4]; c.k2 = v[5]; c.p1 = v[6]; c.p2 = v[7]; c.k3 = v[8]; c.k4 = v[9]; c.k5 = v[10]; c.k6 = v[11];
  c.max_r = v[12];
  return c;
}

int main(int argc, char** argv) {
  if (argc < 4) {
    cerr << "usage: " << argv[0] << " depth.u16 scale calib.f64" << endl;
    return 1;
  }
  try {
    const size_t n_calib = 2 + 13 + 2 + 13 + 9 + 3;
    vector<double> cal(n_calib + 1);
    read_raw(argv[3], cal, n_calib);
    const int dRows = (int)cal[0], dCols = (int)cal[1], cRows = (int)cal[15], cCols = (int)cal[16];
    if (dRows <= 0 || dCols <= 0) throw ppf_match_3d::Error(PPF_ERR_INVALID, "calib.f64: the depth image has no pixels");
    vector<uint16_t> depth((size_t)dRows * dCols + 1);
    read_raw(argv[1], depth, (size_t)dRows * dCols);

    /* once per calibration */
    const prep::DepthMap map(camera_of(&cal[2]), dRows, dCols, camera_of(&cal[17]), cRows, cCols, &cal[30], &cal[39]);
    /* per frame: the aligned image, then Deprojection on it */
    ppf_register_stats st;
    const vector<float> aligned = map.registerDepthU16(&depth[0], atof(argv[2]), 0.f, 0.f, 0, 0, &st);
    printf("registered vertices %d quads %d cut %d oversize %d filled %d launches %d\n", (int)st.n_vertices, (int)st.n_quads,
           (int)st.n_quads_cut, (int)st.n_quads_oversize, (int)st.n_filled, (int)st.n_launches);
    const prep::Cloud scene = prep::Cloud::fromDepth(aligned.empty() ? 0 : &aligned[0], map.rows(), map.cols(), map.fx(), map.fy(),
                                                     map.ppx(), map.ppy());
    printf("scene_points %d\n", scene.size());
  } catch (const ppf_match_3d::Error& e) {
    cerr << e.what() << endl;
    return 10 + e.status;
  }
  return 0;
}
