/* ORACLE — TEST INFRASTRUCTURE ONLY.  oracle_raytrace_ext and the four array entry points of the shading extensions in a program of
 * its own for the address and undefined-behaviour sanitizers (make -C oracle shading-ext-check; tests/test_shading_ext_cpu.py runs
 * it): a closed room whose walls read three textures (two with chains, one nearest) through an atlas allocated to the texel, so
 * that a tap or a level outside it is a heap overflow; mirror, glossy and diffuse records shared by "instances" (n_base 4 of 12
 * triangles); two samples per pixel with every dump plane; then the same without a level table on a strip; then the samplers, the
 * bounce and the footprint on hostile operands (NaN, infinities, levels beyond the chain). */
#include "rtpt_oracle.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
static float frand(unsigned* s) { *s = *s * 1664525u + 1013904223u; return (float)(*s >> 8) / 16777216.0f; }
int main(void) {
  unsigned seed = 7;
  /* a closed box of 12 triangles around the camera, 3 instances' worth of ids via n_base = 4 */
  float lo[3] = {-2, -1, -3}, hi[3] = {2, 1, 1};
  float q[6][4][3] = {
      {{lo[0], lo[1], lo[2]}, {lo[0], lo[1], hi[2]}, {lo[0], hi[1], hi[2]}, {lo[0], hi[1], lo[2]}},
      {{hi[0], lo[1], lo[2]}, {hi[0], hi[1], lo[2]}, {hi[0], hi[1], hi[2]}, {hi[0], lo[1], hi[2]}},
      {{lo[0], lo[1], lo[2]}, {hi[0], lo[1], lo[2]}, {hi[0], lo[1], hi[2]}, {lo[0], lo[1], hi[2]}},
      {{lo[0], hi[1], lo[2]}, {lo[0], hi[1], hi[2]}, {hi[0], hi[1], hi[2]}, {hi[0], hi[1], lo[2]}},
      {{lo[0], lo[1], lo[2]}, {lo[0], hi[1], lo[2]}, {hi[0], hi[1], lo[2]}, {hi[0], lo[1], lo[2]}},
      {{lo[0], lo[1], hi[2]}, {hi[0], lo[1], hi[2]}, {hi[0], hi[1], hi[2]}, {lo[0], hi[1], hi[2]}}};
  float tris[12 * 9];
  for (int w = 0; w < 6; w++) {
    int a[2][3] = {{0, 1, 2}, {0, 2, 3}};
    for (int t = 0; t < 2; t++)
      for (int k = 0; k < 3; k++) memcpy(tris + 9 * (2 * w + t) + 3 * k, q[w][a[t][k]], 12);
  }
  enum { NB = 4, NT = 3 };
  float mat[NB * 8] = {0};
  for (int i = 0; i < NB; i++) { mat[8 * i] = 0.5f; mat[8 * i + 1] = 0.75f; mat[8 * i + 2] = 0.25f; }
  mat[8 * 1 + 3] = -0.0f; mat[8 * 2 + 3] = -0.3f; mat[8 * 3 + 3] = -1.0f;
  float uv[NB * 6];
  for (int i = 0; i < NB * 6; i++) uv[i] = -2.5f + 6.0f * frand(&seed);
  uint32_t tt[NB] = {1, 2, 3, 0};
  /* textures: 33 x 17 with a chain, 16 x 4 nearest with a chain, 3 x 5 without */
  uint32_t dims[NT][2] = {{33, 17}, {16, 4}, {3, 5}};
  uint32_t flags[NT] = {ORACLE_TEX_MIPMAP, ORACLE_TEX_MIPMAP | ORACLE_TEX_NEAREST, 0};
  uint32_t desc[NT * 4], rows[NT * ORACLE_TEX_LEVEL_ROW];
  memset(rows, 0, sizeof rows);
  uint32_t total = 0;
  for (int t = 0; t < NT; t++) {
    desc[4 * t] = dims[t][0]; desc[4 * t + 1] = dims[t][1]; desc[4 * t + 2] = total; desc[4 * t + 3] = flags[t];
    uint32_t w = dims[t][0], h = dims[t][1], l = 0;
    for (;;) {
      rows[ORACLE_TEX_LEVEL_ROW * t + l++] = total;
      total += w * h;
      if (!(flags[t] & ORACLE_TEX_MIPMAP) || (w == 1 && h == 1)) break;
      w = w > 1 ? w >> 1 : 1; h = h > 1 ? h >> 1 : 1;
    }
    rows[ORACLE_TEX_LEVEL_ROW * t + ORACLE_TEX_MAX_LEVELS] = l;
  }
  float* texels = malloc(16 * (size_t)total); /* exactly the atlas: a tap outside it is a heap overflow */
  for (uint32_t i = 0; i < 4 * total; i++) texels[i] = frand(&seed);
  enum { W = 97, H = 13, SEG = 9, SPP = 2 };
  oracle_config cfg;
  oracle_config_default(&cfg, W, H);
  cfg.max_segments = SEG; cfg.samples_per_pixel = SPP;
  oracle_push_constants pc;
  memset(&pc, 0, sizeof pc);
  pc.cameraPos[0] = 0.1f; pc.cameraPos[1] = -0.05f; pc.cameraPos[2] = 0.5f;
  pc.lightPos[0] = 300; pc.lightPos[1] = 5000; pc.lightPos[2] = -400;
  pc.currentCameraColor[0] = pc.currentCameraColor[1] = pc.currentCameraColor[2] = 0.5f;
  size_t np = (size_t)W * H, nr = np * SEG * SPP;
  float* image = calloc(np * 4, 4); uint32_t* hit = calloc(np, 4); float* albedo = calloc(np * 4, 4);
  uint16_t* seq_id = calloc(nr, 2); int32_t* seq_n = calloc(np, 4); uint8_t* seq_end = calloc(np, 1); float* dir0 = calloc(np * 3, 4);
  float* rec_lod = calloc(nr, 4); uint8_t* rec_code = calloc(nr, 1); float* rec_alb = calloc(nr * 3, 4); float* rec_ray = calloc(nr * 6, 4);
  oracle_seq_dump dump = {seq_id, seq_n, seq_end, SEG * SPP, dir0};
  oracle_shade_ext ext = {uv, tt, desc, texels, rows, 0.125f, 1, albedo, rec_lod, rec_code, rec_alb, rec_ray};
  uint64_t rays = 0;
  oracle_set_threads(4);
  oracle_raytrace_ext(&cfg, &pc, tris, 12, mat, NB, 0, H, image, &rays, hit, &dump, &ext);
  ext.levels = NULL;
  oracle_raytrace_ext(&cfg, &pc, tris, 12, mat, NB, 2, 7, image, &rays, hit, NULL, &ext);
  unsigned absorbed = 0, tex = 0;
  for (size_t i = 0; i < np; i++) absorbed += seq_end[i] == ORACLE_END_ABSORBED;
  for (size_t i = 0; i < nr; i++) tex += (rec_code[i] & ORACLE_REC_TEXTURED) != 0;
  /* the array entry points on hostile operands */
  float huv[] = {0, 0, 1, 1, -0.0f, 1e6f, -1e6f, 0.5f, NAN, INFINITY, -INFINITY, 3.4e38f, -1e-9f, 1.0f - 1e-7f};
  float lods[] = {-1, 0, 0.5f, 1, 5, 5.5f, 6, 40, NAN, INFINITY, -INFINITY, 1e30f, -0.0f, 2.999999f};
  float out[4 * 7];
  for (int t = 0; t < NT; t++) {
    oracle_texture_sample_array(desc + 4 * t, texels, huv, 7, out);
    for (int k = 0; k < 14; k++) {
      float l7[7]; for (int j = 0; j < 7; j++) l7[j] = lods[(k + j) % 14];
      oracle_texture_sample_lod_array(desc + 4 * t, rows + ORACLE_TEX_LEVEL_ROW * t, texels, huv, l7, 7, out);
    }
  }
  float cases[9 * 3] = {0, -1, 0, 0, 1, 0, 0.25f, 0.5f, 0.3f, 1, 0, 0, 0, 0, 1, 0, 1, 1, NAN, 0, 0, 0, 0, 0, 0.5f, 0.5f, 0};
  oracle_bounce_array(cases, 3, out);
  float fp[17 * 2] = {0.1f, -0.5f, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  oracle_texture_footprint_array(fp, 2, 33, 17, out);
  void* bufs[] = {texels, image, hit, albedo, seq_id, seq_n, seq_end, dir0, rec_lod, rec_code, rec_alb, rec_ray};
  for (size_t i = 0; i < sizeof bufs / sizeof bufs[0]; i++) free(bufs[i]);
  printf("shading_ext_check: rays %llu, absorbed %u, textured records %u, footprint %g %g\n", (unsigned long long)rays, absorbed, tex,
         (double)out[0], (double)out[1]);
  if (!(absorbed > 0 && tex > 1000 && out[0] > 0.0f && out[1] == 0.0f)) return 1;
  printf("shading_ext_check: ok\n");
  return 0;
}
