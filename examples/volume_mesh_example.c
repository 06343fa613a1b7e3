/* The volume's surface as a triangle mesh through the C ABI, from C99: two frames fused into a volume, the volume meshed, saved,
 * restored and meshed again.
 *   match      the second frame aligned against the first: the transformation, as returned, is the second frame's pose in the
 *              first frame's world
 *   integrate  both frames in one call (dvo_amd_volume_integrate, the anonymous form: nothing is kept, so the volume can be restored)
 *   mesh       the surface by surface nets (dvo_amd_volume_mesh): the sizes are asked for first, then the arrays are filled
 *   restore    the records downloaded (dvo_amd_volume_download), put into a fresh volume (dvo_amd_volume_upload) and meshed again:
 *              the same mesh, bit for bit
 *   ply        the mesh written as a PLY file when a path is given (dvo_amd_write_ply)
 * Prints counts and checksums -- what examples/volume_mesh_adaptor_example.cpp prints through the C++ adaptor.  Input files:
 * float32 planes without a header, as tests/test_volume_mesh_adaptor.py writes them.
 *   cc -std=c99 -Iinclude examples/volume_mesh_example.c -Ldvo_slam_amd -ldvo_amd -Wl,-rpath,$PWD/dvo_slam_amd */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dvo_amd.h"

static void *read_file(const char *path, size_t bytes) {
  void *p = malloc(bytes);
  FILE *f = fopen(path, "rb");
  if (!p || !f || fread(p, 1, bytes, f) != bytes) {
    fprintf(stderr, "cannot read %s\n", path);
    exit(2);
  }
  fclose(f);
  return p;
}

#define CHECK(call)                                                                                         \
  do {                                                                                                      \
    int rc_ = (call);                                                                                       \
    if (rc_ != DVO_AMD_OK) {                                                                                \
      fprintf(stderr, "%s: %s [%s]\n", #call, dvo_amd_status_string(rc_), dvo_amd_last_error());             \
      return 1;                                                                                             \
    }                                                                                                       \
  } while (0)

typedef struct {
  dvo_amd_point *vertices;
  float *normals;
  int *triangles;
  dvo_amd_volume_mesh_counts counts;
} mesh;

/* the sizes first, then the arrays */
static int mesh_of(dvo_amd_volume *vol, mesh *m) {
  memset(m, 0, sizeof(*m));
  int rc = dvo_amd_volume_mesh(vol, 1, NULL, NULL, 0, NULL, 0, &m->counts);
  if (rc != DVO_AMD_OK && rc != DVO_AMD_ERR_CAPACITY) return rc;
  const size_t nv = (size_t)m->counts.vertices, nt = (size_t)m->counts.triangles;
  m->vertices = malloc(sizeof(dvo_amd_point) * (nv ? nv : 1));
  m->normals = malloc(3 * sizeof(float) * (nv ? nv : 1));
  m->triangles = malloc(3 * sizeof(int) * (nt ? nt : 1));
  if (!m->vertices || !m->normals || !m->triangles) return DVO_AMD_ERR_OUT_OF_MEMORY;
  return dvo_amd_volume_mesh(vol, 1, m->vertices, m->normals, (long long)nv, m->triangles, (long long)nt, &m->counts);
}

static void mesh_free(mesh *m) { free(m->vertices), free(m->normals), free(m->triangles); }

int main(int argc, char **argv) {
  if (argc < 11) {
    fprintf(stderr, "usage: %s w h fx fy ox oy first_i first_z second_i second_z [surface.ply]\n", argv[0]);
    return 2;
  }
  const int w = atoi(argv[1]), h = atoi(argv[2]);
  const float fx = (float)atof(argv[3]), fy = (float)atof(argv[4]), ox = (float)atof(argv[5]), oy = (float)atof(argv[6]);
  const size_t n = (size_t)w * (size_t)h;
  float *planes[4];
  for (int k = 0; k < 4; ++k) planes[k] = read_file(argv[7 + k], 4 * n);

  dvo_amd_config cfg;
  dvo_amd_default_config(&cfg);
  const int levels = cfg.first_level + 1;
  dvo_amd_context *ctx = NULL;
  dvo_amd_pyramid *frames[2] = {NULL, NULL};
  CHECK(dvo_amd_context_create(0, &cfg, &ctx));
  CHECK(dvo_amd_pyramid_create(0, planes[0], planes[1], w, h, w, fx, fy, ox, oy, levels, 0.0, &frames[0]));
  CHECK(dvo_amd_pyramid_create(0, planes[2], planes[3], w, h, w, fx, fy, ox, oy, levels, 1.0, &frames[1]));

  dvo_amd_result res;
  memset(&res, 0, sizeof(res));
  CHECK(dvo_amd_match(ctx, frames[0], frames[1], NULL, &res));

  dvo_amd_volume_options vopt;
  dvo_amd_default_volume_options(&vopt);
  dvo_amd_volume *vol = NULL, *copy = NULL;
  CHECK(dvo_amd_volume_create(0, &vopt, &vol));
  double poses[32];
  memset(poses, 0, sizeof(poses));
  poses[0] = poses[5] = poses[10] = poses[15] = 1.0;
  memcpy(poses + 16, res.transformation, 16 * sizeof(double));
  const dvo_amd_pyramid *both[2] = {frames[0], frames[1]};
  CHECK(dvo_amd_volume_integrate(vol, 2, both, 0, poses, 1, NULL));

  mesh m, again;
  CHECK(mesh_of(vol, &m));
  printf("mesh counts %lld %lld %lld %lld %lld\n", m.counts.vertices, m.counts.triangles, m.counts.open_edges, m.counts.uncoloured,
         m.counts.flat);
  double sum = 0.0, along = 0.0;
  long long indices = 0;
  for (long long i = 0; i < m.counts.vertices; ++i) sum += m.vertices[i].x, along += m.normals[3 * i + 2];
  for (long long i = 0; i < 3 * m.counts.triangles; ++i) indices += m.triangles[i];
  printf("mesh checksum %.17g %.17g %lld\n", sum, along, indices);

  long long n_records = 0;
  const long long n_voxels = (long long)vopt.nx * vopt.ny * vopt.nz;
  dvo_amd_volume_voxel *records = malloc(sizeof(dvo_amd_volume_voxel) * (size_t)n_voxels);
  if (!records) return 2;
  CHECK(dvo_amd_volume_download(vol, NULL, records, n_voxels, &n_records));
  CHECK(dvo_amd_volume_create(0, &vopt, &copy));
  CHECK(dvo_amd_volume_upload(copy, NULL, records, n_records));
  CHECK(mesh_of(copy, &again));
  const int same = memcmp(&m.counts, &again.counts, sizeof(m.counts)) == 0 &&
                   memcmp(m.vertices, again.vertices, sizeof(dvo_amd_point) * (size_t)m.counts.vertices) == 0 &&
                   memcmp(m.normals, again.normals, 3 * sizeof(float) * (size_t)m.counts.vertices) == 0 &&
                   memcmp(m.triangles, again.triangles, 3 * sizeof(int) * (size_t)m.counts.triangles) == 0;
  printf("restore same %d\n", same);
  if (argc > 11) CHECK(dvo_amd_write_ply(argv[11], m.vertices, m.normals, m.counts.vertices, m.triangles, m.counts.triangles));

  mesh_free(&m), mesh_free(&again);
  free(records);
  dvo_amd_volume_destroy(copy);
  dvo_amd_volume_destroy(vol);
  dvo_amd_pyramid_release(frames[0]);
  dvo_amd_pyramid_release(frames[1]);
  dvo_amd_context_destroy(ctx);
  for (int k = 0; k < 4; ++k) free(planes[k]);
  return 0;
}
