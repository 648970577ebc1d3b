// main.cpp -- headless command line front end with the reference's flags
// (src/main.cpp:34-58: -w -h --scene --scale --flip_yz) plus the knobs the GUI
// exposed (--bounces, --furnace, aperture/focus) and --spp / --out for batch use.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <limits>
#include <map>
#include <string>
#include "render.hpp"

static void WritePFM(const char* path, const std::vector<float>& rgba, unsigned w, unsigned h)
{
    FILE* f = fopen(path, "wb");
    if (!f) return;
    fprintf(f, "PF\n%u %u\n-1.0\n", w, h);
    for (unsigned y = h; y-- > 0;)            // PFM stores the bottom row first
        for (unsigned x = 0; x < w; ++x) fwrite(&rgba[((size_t)y * w + x) * 4], sizeof(float), 3, f);
    fclose(f);
}

int main(int argc, char** argv)
{
    try
    {
        unsigned width = 1280, height = 720, spp = 16, bounces = 3, gpus = 1, frames = 0, samples_ahead = 1;
        std::string scene_path = "assets/ShaderBalls.obj", out, save_cache;
        float scale = 1.0f, aperture = 0.0f, focus = 10.0f;
        bool flip_yz = false, furnace = false, tiled_path = false, shared_device = false, plan_only = false, resolve = true;
        unsigned scene_options = 0;      // rt::Scene::Options (opt-in extensions)
        int filter_iterations = -1;      // --filter n: the spatial filter (rt_frame_filter); -1 = off
        rt_filter_desc filter = RT_FILTER_DESC_DEFAULT;
        int temporal_iterations = -1;    // --temporal_filter n: the temporal filter (rt_frame_filter_temporal); -1 = off
        rt_temporal_filter_desc temporal = RT_TEMPORAL_FILTER_DESC_DEFAULT;
        bool moving = false;             // --camera_step dx,dy,dz: the camera moves by that much every --frames frame
        float camera_step[3] = {0.0f, 0.0f, 0.0f};
        struct ObjectStep { unsigned object; float d[3]; };
        std::vector<ObjectStep> object_steps;   // --object_step i,dx,dy,dz (repeatable): frame k poses object i by the translation k * (dx,dy,dz)
        struct PickAt { unsigned x, y; };
        std::vector<PickAt> picks;              // --pick x,y (repeatable): after the scene is uploaded and posed, print what lies under that pixel
        std::vector<PickAt> picks_all;          // --pick_all x,y (repeatable): every surface under that pixel, nearest first, one line per surface
        bool nearest_signed = false;            // --signed 1: --nearest also prints whether the point is inside (exits outnumber entries along (0.36, 0.48, 0.8))
        std::string ao_out;                     // --ao out.pfm: after the scene is uploaded and posed, write the ambient occlusion image of the camera (grey, RGB equal)
        rt_bake_desc ao = {64u, 0u, 0u, 1e-3f, 1.0f};   // --ao_samples n --ao_radius r --ao_bias b
        std::string ao_atlas_out;               // --ao_atlas out.pfm: after the scene is uploaded and posed, bake the ambient occlusion into a UV atlas (grey, NaN where uncovered)
        rt_atlas_desc atlas = {0u, 0u, 0u, RT_INVALID_ID};   // --atlas_size w,h --atlas_gutter n
        std::string lightmap_out;               // --lightmap out.pfm: after the scene is uploaded and posed, bake the direct irradiance (sky + lights) into a UV atlas (RGB, NaN where uncovered)
        bool atlas_synthetic = false;           // --atlas_uv synthetic: a crack-free grid of two triangles per cell instead of the triangles' own UVs (scenes.synthetic_atlas)
        struct WithinAt { rt_point point; std::uint32_t k; };
        std::vector<WithinAt> within_points;    // --within x,y,z,r[,k] (repeatable): after the scene is uploaded and posed, print the triangles within r (the k nearest only)
        struct OverlapAt { float lo[3], hi[3]; std::uint32_t k; };
        struct CrossAt { rt_probe probe; std::uint32_t k; };
        std::vector<CrossAt> cross_probes;      // --cross x1,y1,z1,x2,y2,z2,x3,y3,z3[,k] (repeatable): after the scene is uploaded and posed, print the triangles that triangle crosses (the k lowest ids)
        struct SeparationAt { rt_probe probe; float r; };
        std::vector<SeparationAt> separation_probes;   // --separation x1,y1,z1,x2,y2,z2,x3,y3,z3[,r] (repeatable): after the scene is uploaded and posed, print the nearest triangle to that triangle (within r), the distance and the two closest points
        bool clearance = false;                 // --clearance 1: print, per object, the nearest other object, the distance and the two closest points
        bool self_cross = false;                // --self_cross 1: print which triangles of the scene cross each other, neighbours that share a corner aside
        std::vector<OverlapAt> overlap_boxes;   // --overlap lx,ly,lz,hx,hy,hz[,k] (repeatable): after the scene is uploaded and posed, print the triangles the box touches (the k lowest ids)
        struct RectAt { std::uint32_t x0, y0, x1, y1; bool window; };
        std::vector<RectAt> pick_rects;         // --pick_rect x0,y0,x1,y1[,window] (repeatable): print what lies under that pixel rectangle (window: wholly inside it)
        std::vector<rt_point> nearest_points;   // --nearest x,y,z[,r] (repeatable): after the scene is uploaded and posed, print the nearest surface point (within r)
        bool list_objects = false;              // --list_objects 1: print the OBJ's o / g shapes (index and name) and exit; needs no GPU
        for (int i = 1; i < argc; ++i)
        {
            auto next = [&]() -> const char* { if (i + 1 >= argc) { std::cerr << "missing value for " << argv[i] << "\n"; exit(2); } return argv[++i]; };
            if (!strcmp(argv[i], "-w")) width = (unsigned)atoi(next());
            else if (!strcmp(argv[i], "-h")) height = (unsigned)atoi(next());
            else if (!strcmp(argv[i], "--scene")) scene_path = next();
            else if (!strcmp(argv[i], "--scale")) scale = (float)atof(next());
            else if (!strcmp(argv[i], "--flip_yz")) flip_yz = atoi(next()) != 0;
            else if (!strcmp(argv[i], "--spp")) spp = (unsigned)atoi(next());
            else if (!strcmp(argv[i], "--bounces")) bounces = (unsigned)atoi(next());
            else if (!strcmp(argv[i], "--furnace")) furnace = atoi(next()) != 0;
            else if (!strcmp(argv[i], "--aperture")) aperture = (float)atof(next());
            else if (!strcmp(argv[i], "--focus")) focus = (float)atof(next());
            else if (!strcmp(argv[i], "--out")) out = next();
            else if (!strcmp(argv[i], "--save-cache")) save_cache = next();
            else if (!strcmp(argv[i], "--gpus")) gpus = (unsigned)atoi(next());
            else if (!strcmp(argv[i], "--resolve")) resolve = atoi(next()) != 0;          // with --frames: 0 = no ResolveRadiance / present per frame (diagnostic)
            else if (!strcmp(argv[i], "--frames")) frames = (unsigned)atoi(next());      // the reference's interactive loop, headless: n x RenderFrame()
            else if (!strcmp(argv[i], "--samples_ahead")) samples_ahead = (unsigned)atoi(next());   // with --frames: RT_OPT_SAMPLES_AHEAD (1 = the integrator's default, 0 = off)
            else if (!strcmp(argv[i], "--tiled")) tiled_path = atoi(next()) != 0;      // take the TiledRender path even with one GPU
            else if (!strcmp(argv[i], "--shared_device")) shared_device = atoi(next()) != 0;   // all tiles on GPU 0 (device copies instead of RCCL)
            else if (!strcmp(argv[i], "--plan")) plan_only = atoi(next()) != 0;              // print the tiling and exit: no GPU, no scene
            else if (!strcmp(argv[i], "--wide_texture_indices")) { if (atoi(next()) != 0) scene_options |= rt::Scene::kWideTextureIndices; }
            else if (!strcmp(argv[i], "--emissive_nee")) { if (atoi(next()) != 0) scene_options |= rt::Scene::kEmissiveNee; }
            else if (!strcmp(argv[i], "--filter")) filter_iterations = atoi(next());          // the spatial filter with n iterations; --out writes the filtered image
            else if (!strcmp(argv[i], "--filter_sigmas"))
            {
                const char* v = next();
                if (sscanf(v, "%f,%f,%f", &filter.sigma_color, &filter.sigma_normal, &filter.sigma_depth) != 3)
                {
                    std::cerr << "--filter_sigmas wants c,n,z (three numbers)\n";
                    return 2;
                }
            }
            else if (!strcmp(argv[i], "--temporal_filter")) temporal_iterations = atoi(next());   // the temporal filter with n iterations
            else if (!strcmp(argv[i], "--temporal_alphas"))
            {
                const char* v = next();
                if (sscanf(v, "%f,%f", &temporal.alpha_color, &temporal.alpha_moments) != 2)
                {
                    std::cerr << "--temporal_alphas wants c,m (two numbers)\n";
                    return 2;
                }
            }
            else if (!strcmp(argv[i], "--temporal_sigmas"))
            {
                const char* v = next();
                if (sscanf(v, "%f,%f,%f", &temporal.sigma_luminance, &temporal.sigma_normal, &temporal.sigma_depth) != 3)
                {
                    std::cerr << "--temporal_sigmas wants l,n,z (three numbers)\n";
                    return 2;
                }
            }
            else if (!strcmp(argv[i], "--camera_step"))
            {
                const char* v = next();
                if (sscanf(v, "%f,%f,%f", &camera_step[0], &camera_step[1], &camera_step[2]) != 3)
                {
                    std::cerr << "--camera_step wants dx,dy,dz (three numbers)\n";
                    return 2;
                }
                moving = true;
            }
            else if (!strcmp(argv[i], "--object_step"))
            {
                ObjectStep s;
                if (sscanf(next(), "%u,%f,%f,%f", &s.object, &s.d[0], &s.d[1], &s.d[2]) != 4)
                {
                    std::cerr << "--object_step wants i,dx,dy,dz (an object index and three numbers)\n";
                    return 2;
                }
                object_steps.push_back(s);
                scene_options |= rt::Scene::kObjects;
            }
            else if (!strcmp(argv[i], "--pick"))
            {
                PickAt p;
                if (sscanf(next(), "%u,%u", &p.x, &p.y) != 2) { std::cerr << "--pick wants x,y (image coordinates)\n"; return 2; }
                picks.push_back(p);
                scene_options |= rt::Scene::kObjects;
            }
            else if (!strcmp(argv[i], "--pick_all"))
            {
                PickAt p;
                if (sscanf(next(), "%u,%u", &p.x, &p.y) != 2) { std::cerr << "--pick_all wants x,y (image coordinates)\n"; return 2; }
                picks_all.push_back(p);
                scene_options |= rt::Scene::kObjects;
            }
            else if (!strcmp(argv[i], "--signed")) nearest_signed = atoi(next()) != 0;
            else if (!strcmp(argv[i], "--nearest"))
            {
                rt_point q;
                q.max_distance = INFINITY;
                if (sscanf(next(), "%f,%f,%f,%f", &q.position[0], &q.position[1], &q.position[2], &q.max_distance) < 3)
                {
                    std::cerr << "--nearest wants x,y,z or x,y,z,r (a point and an optional largest distance)\n";
                    return 2;
                }
                nearest_points.push_back(q);
                scene_options |= rt::Scene::kObjects;
            }
            else if (!strcmp(argv[i], "--within"))
            {
                WithinAt q;
                q.k = 0u;
                const int got = sscanf(next(), "%f,%f,%f,%f,%u", &q.point.position[0], &q.point.position[1], &q.point.position[2], &q.point.max_distance, &q.k);
                if (got < 4 || (got == 5 && (q.k < 1u || q.k > RT_WITHIN_MAX)))
                {
                    std::cerr << "--within wants x,y,z,r or x,y,z,r,k (a point, a radius and optionally how many of the nearest to look for, 1 .. 8)\n";
                    return 2;
                }
                within_points.push_back(q);
                scene_options |= rt::Scene::kObjects;
            }
            else if (!strcmp(argv[i], "--cross"))
            {
                CrossAt q = {};
                q.k = RT_CROSS_LIST_MAX;
                float* p[3] = {q.probe.p1, q.probe.p2, q.probe.p3};
                const int got = sscanf(next(), "%f,%f,%f,%f,%f,%f,%f,%f,%f,%u", &p[0][0], &p[0][1], &p[0][2], &p[1][0], &p[1][1], &p[1][2], &p[2][0], &p[2][1], &p[2][2], &q.k);
                if (got < 9 || q.k > RT_CROSS_LIST_MAX)
                {
                    std::cerr << "--cross wants x1,y1,z1,x2,y2,z2,x3,y3,z3 or the same followed by ,k (a triangle's corners and optionally how many triangles to list, 0 .. 8)\n";
                    return 2;
                }
                cross_probes.push_back(q);
                scene_options |= rt::Scene::kObjects;
            }
            else if (!strcmp(argv[i], "--separation"))
            {
                SeparationAt q = {};
                q.r = std::numeric_limits<float>::infinity();
                float* p[3] = {q.probe.p1, q.probe.p2, q.probe.p3};
                const int got = sscanf(next(), "%f,%f,%f,%f,%f,%f,%f,%f,%f,%f", &p[0][0], &p[0][1], &p[0][2], &p[1][0], &p[1][1], &p[1][2], &p[2][0], &p[2][1], &p[2][2], &q.r);
                if (got < 9 || !(q.r >= 0.0f))
                {
                    std::cerr << "--separation wants x1,y1,z1,x2,y2,z2,x3,y3,z3 or the same followed by ,r (a triangle's corners and optionally the largest distance searched, >= 0)\n";
                    return 2;
                }
                separation_probes.push_back(q);
                scene_options |= rt::Scene::kObjects;
            }
            else if (!strcmp(argv[i], "--clearance")) { if (atoi(next()) != 0) { clearance = true; scene_options |= rt::Scene::kObjects; } }
            else if (!strcmp(argv[i], "--self_cross")) { if (atoi(next()) != 0) { self_cross = true; scene_options |= rt::Scene::kObjects; } }
            else if (!strcmp(argv[i], "--overlap"))
            {
                OverlapAt q;
                q.k = RT_REGION_LIST_MAX;
                const int got = sscanf(next(), "%f,%f,%f,%f,%f,%f,%u", &q.lo[0], &q.lo[1], &q.lo[2], &q.hi[0], &q.hi[1], &q.hi[2], &q.k);
                if (got < 6 || q.k > RT_REGION_LIST_MAX)
                {
                    std::cerr << "--overlap wants lx,ly,lz,hx,hy,hz or lx,ly,lz,hx,hy,hz,k (a box's corners and optionally how many triangles to list, 0 .. 8)\n";
                    return 2;
                }
                overlap_boxes.push_back(q);
                scene_options |= rt::Scene::kObjects;
            }
            else if (!strcmp(argv[i], "--pick_rect"))
            {
                RectAt q;
                char word[16] = "";
                const int got = sscanf(next(), "%u,%u,%u,%u,%15s", &q.x0, &q.y0, &q.x1, &q.y1, word);
                q.window = got == 5 && !strcmp(word, "window");
                if (got < 4 || (got == 5 && !q.window))
                {
                    std::cerr << "--pick_rect wants x0,y0,x1,y1 or x0,y0,x1,y1,window (an inclusive pixel rectangle; window: only what lies wholly inside it)\n";
                    return 2;
                }
                pick_rects.push_back(q);
                scene_options |= rt::Scene::kObjects;
            }
            else if (!strcmp(argv[i], "--ao")) ao_out = next();
            else if (!strcmp(argv[i], "--ao_atlas")) ao_atlas_out = next();
            else if (!strcmp(argv[i], "--lightmap")) lightmap_out = next();
            else if (!strcmp(argv[i], "--atlas_size")) { if (sscanf(next(), "%u,%u", &atlas.width, &atlas.height) != 2) { std::cerr << "--atlas_size w,h\n"; return 2; } }
            else if (!strcmp(argv[i], "--atlas_gutter")) atlas.gutter = (unsigned)atoi(next());
            else if (!strcmp(argv[i], "--atlas_uv")) atlas_synthetic = !strcmp(next(), "synthetic");
            else if (!strcmp(argv[i], "--ao_samples")) ao.samples = (unsigned)atoi(next());
            else if (!strcmp(argv[i], "--ao_radius")) ao.radius = (float)atof(next());
            else if (!strcmp(argv[i], "--ao_bias")) ao.bias = (float)atof(next());
            else if (!strcmp(argv[i], "--list_objects")) { if (atoi(next()) != 0) { list_objects = true; scene_options |= rt::Scene::kObjects; } }
            else if (!strcmp(argv[i], "--help"))
            {
                std::cout << "rt_render -w W -h H --scene file.obj [--scale s] [--flip_yz 0|1] [--spp n] [--bounces b]"
                             " [--furnace 0|1] [--aperture a] [--focus d] [--out image.pfm] [--save-cache scene.rtscene] [--gpus n]\n"
                             "  --gpus n tiles the image over devices 0..n-1 (interleaved 8-row bands, one RCCL gather);\n"
                             "  --shared_device 1 puts all n tiles on GPU 0 (device copies instead of RCCL); --plan 1 prints the tiling and exits\n"
                             "  --scene also accepts a file written by --save-cache (parsed scene + BVH)\n"
                             "  --frames n times the reference's own loop instead of a batch: n x Render::RenderFrame() = one Integrate() through\n"
                             "  the fifteen hooks, one sample per pixel, ResolveRadiance + Finish() every frame (src/render.cpp:172-204);\n"
                             "  --samples_ahead 0 makes every one of them trace its own sample (default 1: a standing camera's next samples are traced ahead in batches)\n"
                             "  extensions (off = the reference's behaviour): --wide_texture_indices 1 loads scenes with more than 255\n"
                             "  textures; --emissive_nee 1 adds the emissive triangles to next-event estimation\n"
                             "  --filter n [--filter_sigmas c,n,z] runs the spatial filter (n a-trous iterations, 0 .. 8; sigmas default to\n"
                             "  RT_FILTER_DESC_DEFAULT's) and --out then writes the filtered, tone-mapped image; whole images only (not with --gpus > 1)\n"
                             "  --temporal_filter n [--temporal_alphas c,m] [--temporal_sigmas l,n,z] runs the temporal filter (SVGF; n a-trous\n"
                             "  iterations, 0 .. 8; the rest default to RT_TEMPORAL_FILTER_DESC_DEFAULT's) on every frame; whole images only\n"
                             "  --frames n --camera_step dx,dy,dz renders n frames of one sample each, the camera moving by (dx,dy,dz) every frame\n"
                             "  (the reference's moving-camera loop: each frame is reset); --out then writes the last frame's image\n"
                             "  --list_objects 1 prints the scene's objects (the OBJ's o / g shapes: index and name) and exits\n"
                             "  --frames n --object_step i,dx,dy,dz (repeatable) poses object i by the translation k * (dx,dy,dz) in frame k, on the device\n"
                             "  (rt_scene_pose: the scene is uploaded refittable, and with --temporal_filter the history follows the move); one GPU only\n"
                             "  --pick x,y (repeatable) prints what lies under the centre of that pixel once the scene is uploaded and posed: primitive, t, position,\n"
                             "  normals, texture coordinates, material and object (index and name); one GPU only\n"
                             "  --lightmap out.pfm --atlas_size w,h [--atlas_gutter n] [--atlas_uv own|synthetic] bakes the irradiance of the sky and of the scene's lights into a UV atlas (--ao_samples rays per texel; NaN where uncovered)\n"
                             "  --ao_atlas out.pfm --atlas_size w,h [--atlas_gutter n] [--atlas_uv own|synthetic] bakes the ambient occlusion into a UV atlas (--ao_samples / --ao_radius; NaN where uncovered)\n"
                             "  --ao out.pfm --ao_samples n --ao_radius r [--ao_bias b] writes the exact ambient occlusion image of the camera once the scene is uploaded\n"
                             "  and posed: per pixel the share of n cosine-weighted rays (a power of two, 16 .. 4096; default 64) from the first hit that meet nothing within r\n"
                             "  (default 1), 1 where the pixel sees nothing; traced and baked on the device (rt_scene_bake_buffer); one GPU only\n"
                             "  --pick_all x,y (repeatable) prints every surface under that pixel, nearest first, one line per surface; --signed 1 makes --nearest print whether\n"
                             "    the point is inside (more exits than entries along (0.36, 0.48, 0.8))\n"
                             "  --cross x1,y1,z1,x2,y2,z2,x3,y3,z3[,k] (repeatable) prints the triangles that triangle crosses once the scene is uploaded and posed: how many, and\n"
                             "  one line for each of the k (default 8) lowest primitive ids with the two contact points; --self_cross 1 prints how many of the scene's own\n"
                             "  triangles cross another one (neighbours that share a corner aside) and the pairs of objects among them; one GPU only\n"
                             "  --separation x1,y1,z1,x2,y2,z2,x3,y3,z3[,r] (repeatable) prints the nearest triangle to that triangle (within r, default any distance) once the\n"
                             "  scene is uploaded and posed: the distance, the two closest points, the winning feature and the object; --clearance 1 prints, per object, the\n"
                             "  nearest other object, the distance, the two closest points and the two triangles; one GPU only\n"
                             "  --overlap lx,ly,lz,hx,hy,hz[,k] (repeatable) prints the triangles that axis-aligned box touches once the scene is uploaded and posed: how many,\n"
                             "  how many lie wholly inside, and one line for each of the k (default 8) lowest primitive ids; --pick_rect x0,y0,x1,y1[,window] (repeatable)\n"
                             "  prints what lies under that inclusive pixel rectangle: the primitives its region touches (window: wholly inside) and their objects; one GPU only\n"
                             "  --within x,y,z,r[,k] (repeatable) prints the triangles within r of that point once the scene is uploaded and posed: their count, and one line\n"
                             "  for each of the nearest 8 (with k: the k nearest only, and nothing beyond them is looked for)\n"
                             "  --nearest x,y,z[,r] (repeatable) prints the nearest surface point to that point (within r) once the scene is uploaded and posed: primitive,\n"
                             "  distance, position, feature (face, edge or vertex), material and object (index and name); one GPU only\n";
                return 0;
            }
        }
        if (filter_iterations >= 0)
        {
            filter.iterations = (std::uint32_t)filter_iterations;
            if (gpus > 1)
            {
                std::cerr << "--filter needs the whole image on one GPU: not with --gpus > 1\n";
                return 2;
            }
        }
        if (temporal_iterations >= 0)
        {
            temporal.iterations = (std::uint32_t)temporal_iterations;
            if (gpus > 1)
            {
                std::cerr << "--temporal_filter needs the whole image on one GPU: not with --gpus > 1\n";
                return 2;
            }
            if (filter_iterations >= 0)
            {
                std::cerr << "--temporal_filter and --filter exclude each other\n";
                return 2;
            }
        }
        if (moving && frames == 0)
        {
            std::cerr << "--camera_step needs --frames n\n";
            return 2;
        }
        if (!object_steps.empty() && (frames == 0 || gpus > 1 || tiled_path))
        {
            std::cerr << "--object_step needs --frames n and one GPU\n";
            return 2;
        }
        if (!picks_all.empty() && (gpus > 1 || tiled_path))
        {
            std::cerr << "--pick_all needs one GPU\n";
            return 2;
        }
        if (!picks.empty() && (gpus > 1 || tiled_path))
        {
            std::cerr << "--pick needs one GPU\n";
            return 2;
        }
        if (!nearest_points.empty() && (gpus > 1 || tiled_path))
        {
            std::cerr << "--nearest needs one GPU\n";
            return 2;
        }
        if (!within_points.empty() && (gpus > 1 || tiled_path))
        {
            std::cerr << "--within needs one GPU\n";
            return 2;
        }
        if ((!cross_probes.empty() || self_cross) && (gpus > 1 || tiled_path))
        {
            std::cerr << "--cross and --self_cross need one GPU\n";
            return 2;
        }
        if ((!separation_probes.empty() || clearance) && (gpus > 1 || tiled_path))
        {
            std::cerr << "--separation and --clearance need one GPU\n";
            return 2;
        }
        if ((!overlap_boxes.empty() || !pick_rects.empty()) && (gpus > 1 || tiled_path))
        {
            std::cerr << "--overlap and --pick_rect need one GPU\n";
            return 2;
        }
        if (!ao_out.empty() && (gpus > 1 || tiled_path))
        {
            std::cerr << "--ao needs one GPU\n";
            return 2;
        }
        if (plan_only)
        {
            // which rows each GPU renders (TiledRender::TileRows = rt_frame_desc's rule); needs neither a GPU nor the scene
            std::size_t total = 0;
            for (unsigned r = 0; r < gpus; ++r)
            {
                std::vector<std::uint32_t> rows = rt::TiledRender::TileRows(height, r, gpus);
                total += rows.size();
                std::cout << "tile " << r << " of " << gpus << ": " << rows.size() << " rows x " << width << " =";
                for (std::uint32_t y : rows) std::cout << " " << y;
                std::cout << std::endl;
            }
            std::cout << "total rows " << total << " of " << height << std::endl;
            return total == height ? 0 : 1;
        }
        rt::Scene scene(scene_path.c_str(), scale, flip_yz, scene_options);
        scene.AddDirectionalLight({-0.6f, -1.5f, 3.5f}, {15.0f, 10.0f, 5.0f});   // main.cpp:58
        if (list_objects)
        {
            for (std::size_t k = 0; k < scene.GetObjectNames().size(); ++k) std::cout << k << " " << scene.GetObjectNames()[k] << std::endl;
            return 0;
        }
        for (const ObjectStep& s : object_steps)
            if (s.object >= scene.GetObjectNames().size())
            {
                std::cerr << "--object_step: the scene has " << scene.GetObjectNames().size() << " objects (--list_objects 1)\n";
                return 2;
            }
        if (gpus > 1 || tiled_path)
        {
            std::vector<int> devices;
            for (unsigned d = 0; d < gpus; ++d) devices.push_back(shared_device ? 0 : (int)d);
            rt::TiledRender tiled(width, height, scene, devices);
            tiled.SetSpatialFilter(filter_iterations >= 0 ? &filter : nullptr);   // (refuses any filter)
            tiled.SetTemporalFilter(temporal_iterations >= 0 ? &temporal : nullptr);
            for (unsigned d = 0; d < gpus; ++d) std::cout << "tile " << d << " on device " << devices[d] << ": " << tiled.GetContext(d).DeviceName() << std::endl;
            std::cout << "gather: " << (tiled.GetRcclRanks() ? "RCCL ncclGather, communicator of " + std::to_string(tiled.GetRcclRanks()) + " ranks"
                                                              : std::string("device copies on one GPU (local group)")) << std::endl;
            if (!save_cache.empty()) scene.SaveCache(save_cache.c_str(), tiled.GetAccelerationStructure().GetNodes());
            rt::Camera cam = rt::DefaultCamera(width, height);
            cam.aperture = aperture;
            cam.focus_distance = focus;
            tiled.SetCamera(cam);
            tiled.SetMaxBounces(bounces);
            tiled.EnableWhiteFurnace(furnace);
            auto t0 = std::chrono::steady_clock::now();
            tiled.RenderSamples(spp);
            double t_render = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            std::vector<float> sum = tiled.GatherRadiance(0);
            double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            rt_stats st = tiled.GetStats();
            double rays = (double)st.closest_rays + (double)st.shadow_rays;
            std::cout << spp << " spp on " << gpus << " GPUs in " << dt << " s (render " << t_render << " s, gather "
                      << (dt - t_render) * 1e3 << " ms), " << rays / dt / 1e6 << " Mrays/s; tile seconds:";
            for (double t : tiled.GetLastTileSeconds()) std::cout << " " << t;
            std::cout << std::endl;
            if (!out.empty())
            {
                for (float& v : sum) v /= (float)spp;
                WritePFM(out.c_str(), sum, width, height);
            }
            return 0;
        }
        rt::Render render(width, height, scene);
        std::cout << "device: " << render.GetContext().DeviceName() << std::endl;
        if (!save_cache.empty()) scene.SaveCache(save_cache.c_str(), render.GetAccelerationStructure().GetNodes());
        rt::Camera cam = rt::DefaultCamera(width, height);
        cam.aperture = aperture;
        cam.focus_distance = focus;
        render.SetCamera(cam);
        render.GetIntegrator().SetMaxBounces(bounces);
        render.GetIntegrator().EnableWhiteFurnace(furnace);
        render.GetIntegrator().SetSpatialFilter(filter_iterations >= 0 ? &filter : nullptr);
        render.GetIntegrator().SetTemporalFilter(temporal_iterations >= 0 ? &temporal : nullptr);
        // --pick: one line per pixel (rt_frame_pick through Render::Pick); the object is the scene's own table's where none was set on the device
        auto print_picks = [&]()
        {
            for (const PickAt& p : picks)
            {
                rt_hit h; rt_surface s;
                render.Pick(p.x, p.y, nullptr, &h, &s);
                std::cout << "pick " << p.x << "," << p.y << ": ";
                if (s.primitive_id == RT_INVALID_ID) { std::cout << "miss" << std::endl; continue; }
                std::uint32_t object = s.object;
                if (object == RT_INVALID_ID && s.primitive_id < scene.GetTriangleObjects().size()) object = scene.GetTriangleObjects()[s.primitive_id];
                std::cout << "primitive " << s.primitive_id << " t " << s.t << " position " << s.position[0] << " " << s.position[1] << " " << s.position[2]
                          << " geometric_normal " << s.geometric_normal[0] << " " << s.geometric_normal[1] << " " << s.geometric_normal[2]
                          << " shading_normal " << s.shading_normal[0] << " " << s.shading_normal[1] << " " << s.shading_normal[2]
                          << " texcoord " << s.texcoord[0] << " " << s.texcoord[1] << " material " << s.mtl_index << " object ";
                if (object < scene.GetObjectNames().size()) std::cout << object << " " << scene.GetObjectNames()[object];
                else std::cout << "none";
                std::cout << ((s.flags & 2u) ? " (back face)" : "") << std::endl;
            }
        };
        // --pick_all: one line per surface under the pixel, nearest first (rt_scene_trace_all through Render::PickAll); the object as --pick names it
        auto print_picks_all = [&]()
        {
            for (const PickAt& p : picks_all)
            {
                rt_ray_hits rec; rt_hit h[RT_ALL_HITS_MAX]; rt_surface s[RT_ALL_HITS_MAX];
                render.PickAll(p.x, p.y, RT_ALL_HITS_MAX, nullptr, &rec, h, s);
                std::cout << "pick_all " << p.x << "," << p.y << ": " << rec.count << " surfaces, " << rec.entering << " entered" << std::endl;
                for (std::uint32_t j = 0; j < rec.stored; ++j)
                {
                    std::uint32_t object = s[j].object;
                    if (object == RT_INVALID_ID && s[j].primitive_id < scene.GetTriangleObjects().size()) object = scene.GetTriangleObjects()[s[j].primitive_id];
                    std::cout << "  " << j << ": primitive " << s[j].primitive_id << " t " << s[j].t << " position " << s[j].position[0] << " " << s[j].position[1] << " "
                              << s[j].position[2] << " material " << s[j].mtl_index << " object ";
                    if (object < scene.GetObjectNames().size()) std::cout << object << " " << scene.GetObjectNames()[object];
                    else std::cout << "none";
                    std::cout << (((rec.flags >> (RT_RAY_HITS_EXIT_SHIFT + j)) & 1u) ? " (exit)" : "") << std::endl;
                }
            }
        };
        // --nearest: one line per point (rt_scene_nearest through Render::Nearest); the object as --pick names it
        auto print_nearest = [&]()
        {
            if (nearest_points.empty()) return;
            std::vector<rt_nearest> found(nearest_points.size());
            std::vector<rt_surface> surf(nearest_points.size());
            render.Nearest(nearest_points.data(), nearest_points.size(), found.data(), surf.data());
            std::vector<rt_ray_hits> crossed(nearest_points.size());
            if (nearest_signed)
            {
                std::vector<rt_ray> rays(nearest_points.size());
                for (size_t i = 0; i < rays.size(); ++i)
                {
                    const rt_point& q = nearest_points[i];
                    rays[i].origin = {q.position[0], q.position[1], q.position[2], 0.0f};
                    rays[i].direction = {0.36f, 0.48f, 0.8f, RT_MAX_RENDER_DIST};
                }
                render.TraceAllHits(rays.data(), rays.size(), 0u, crossed.data(), nullptr, nullptr);
            }
            for (size_t i = 0; i < found.size(); ++i)
            {
                const rt_point& q = nearest_points[i];
                const rt_nearest& f = found[i];
                std::cout << "nearest " << q.position[0] << "," << q.position[1] << "," << q.position[2] << ": ";
                if (f.primitive_id == RT_INVALID_ID) { std::cout << "none" << std::endl; continue; }
                std::uint32_t object = surf[i].object;
                if (object == RT_INVALID_ID && f.primitive_id < scene.GetTriangleObjects().size()) object = scene.GetTriangleObjects()[f.primitive_id];
                static const char* const feature[4] = {"face", "edge", "vertex", "?"};
                std::cout << "primitive " << f.primitive_id << " distance " << f.distance << " position " << f.position[0] << " " << f.position[1] << " " << f.position[2]
                          << " feature " << feature[(f.flags >> RT_NEAREST_FEATURE_SHIFT) & 3u] << " material " << surf[i].mtl_index << " object ";
                if (object < scene.GetObjectNames().size()) std::cout << object << " " << scene.GetObjectNames()[object];
                else std::cout << "none";
                std::cout << ((f.flags & RT_NEAREST_BACK_SIDE) ? " (back side)" : "");
                if (nearest_signed) std::cout << " inside " << (crossed[i].count - crossed[i].entering > crossed[i].entering ? 1 : 0);
                std::cout << std::endl;
            }
        };
        // --within: one line per point and one per listed member (rt_scene_within through Render::Within); the object as --pick names it
        auto print_within = [&]()
        {
            for (const WithinAt& w : within_points)
            {
                const std::uint32_t k = w.k ? w.k : (std::uint32_t)RT_WITHIN_MAX;
                rt_point_hits rec;
                rt_nearest near[RT_WITHIN_MAX];
                rt_surface surf[RT_WITHIN_MAX];
                render.Within(&w.point, 1, k, w.k ? RT_WITHIN_K_NEAREST : 0u, &rec, near, surf);
                const rt_point& q = w.point;
                std::cout << "within " << q.position[0] << "," << q.position[1] << "," << q.position[2] << " radius " << q.max_distance << ": ";
                if (rec.count == 0u) { std::cout << "none" << std::endl; continue; }
                std::cout << "count " << rec.count << " listed " << rec.stored << " nearest primitive " << rec.nearest_primitive << (w.k ? " (k nearest)" : "") << std::endl;
                for (std::uint32_t j = 0; j < rec.stored; ++j)
                {
                    const rt_nearest& f = near[j];
                    std::uint32_t object = surf[j].object;
                    if (object == RT_INVALID_ID && f.primitive_id < scene.GetTriangleObjects().size()) object = scene.GetTriangleObjects()[f.primitive_id];
                    static const char* const feature[4] = {"face", "edge", "vertex", "?"};
                    std::cout << "within   " << j << ": primitive " << f.primitive_id << " distance " << f.distance << " position " << f.position[0] << " " << f.position[1] << " "
                              << f.position[2] << " feature " << feature[(f.flags >> RT_NEAREST_FEATURE_SHIFT) & 3u] << " material " << surf[j].mtl_index << " object ";
                    if (object < scene.GetObjectNames().size()) std::cout << object << " " << scene.GetObjectNames()[object];
                    else std::cout << "none";
                    std::cout << ((f.flags & RT_NEAREST_BACK_SIDE) ? " (back side)" : "") << std::endl;
                }
            }
        };
        // --overlap: one line per box and one per listed triangle (rt_scene_overlap through Render::Overlap); the object as --pick names it
        auto object_of = [&](std::uint32_t prim) { return prim < scene.GetTriangleObjects().size() ? scene.GetTriangleObjects()[prim] : RT_INVALID_ID; };
        auto print_object = [&](std::uint32_t object)
        {
            if (object < scene.GetObjectNames().size()) std::cout << object << " " << scene.GetObjectNames()[object];
            else std::cout << "none";
        };
        auto print_overlaps = [&]()
        {
            for (const OverlapAt& b : overlap_boxes)
            {
                rt_region g = {};
                g.num_planes = 6u;
                for (int a = 0; a < 3; ++a)
                {
                    g.planes[a][a] = -1.0f; g.planes[a][3] = b.lo[a];                 // lo - x > 0: outside
                    g.planes[3 + a][a] = 1.0f; g.planes[3 + a][3] = -b.hi[a];         // x - hi > 0: outside
                }
                rt_region_hits rec;
                rt_region_member members[RT_REGION_LIST_MAX];
                render.Overlap(&g, 1, b.k, &rec, b.k ? members : nullptr);
                std::cout << "overlap " << b.lo[0] << "," << b.lo[1] << "," << b.lo[2] << " " << b.hi[0] << "," << b.hi[1] << "," << b.hi[2] << ": ";
                if (rec.count == 0u) { std::cout << "none" << std::endl; continue; }
                std::cout << "count " << rec.count << " inside " << rec.inside << " listed " << rec.stored << std::endl;
                for (std::uint32_t j = 0; j < rec.stored; ++j)
                {
                    std::cout << "overlap   " << j << ": primitive " << members[j].primitive_id << ((members[j].flags & RT_REGION_MEMBER_INSIDE) ? " inside" : " crossing") << " object ";
                    print_object(object_of(members[j].primitive_id));
                    std::cout << std::endl;
                }
            }
        };
        // --cross: one line per probe and one per listed triangle (rt_scene_cross through Render::Cross); --self_cross: rt_scene_cross_self over all triangles
        auto print_crosses = [&]()
        {
            for (const CrossAt& q : cross_probes)
            {
                rt_probe_hits rec;
                rt_cross_member members[RT_CROSS_LIST_MAX];
                render.Cross(&q.probe, 1, q.k, 0u, &rec, q.k ? members : nullptr);
                std::cout << "cross " << q.probe.p1[0] << "," << q.probe.p1[1] << "," << q.probe.p1[2] << " " << q.probe.p2[0] << "," << q.probe.p2[1] << "," << q.probe.p2[2] << " "
                          << q.probe.p3[0] << "," << q.probe.p3[1] << "," << q.probe.p3[2] << ": ";
                if (rec.count == 0u) { std::cout << "none" << std::endl; continue; }
                std::cout << "count " << rec.count << " listed " << rec.stored << std::endl;
                for (std::uint32_t j = 0; j < rec.stored; ++j)
                {
                    const rt_cross_member& m = members[j];
                    std::cout << "cross   " << j << ": primitive " << m.primitive_id << " tests " << m.flags << " from " << m.c0[0] << "," << m.c0[1] << "," << m.c0[2] << " to "
                              << m.c1[0] << "," << m.c1[1] << "," << m.c1[2] << " object ";
                    print_object(object_of(m.primitive_id));
                    std::cout << std::endl;
                }
            }
            if (self_cross)
            {
                const std::size_t nt = scene.GetTriangles().size();
                std::vector<rt_probe_hits> recs(nt);
                std::vector<rt_cross_member> members(nt * RT_CROSS_LIST_MAX);
                render.SelfCross(0u, nt, RT_CROSS_LIST_MAX, 0u, recs.data(), members.data());
                std::size_t crossing = 0, listed = 0, over = 0;
                std::vector<std::pair<std::uint32_t, std::uint32_t>> pairs;
                for (std::size_t t = 0; t < nt; ++t)
                {
                    crossing += recs[t].count != 0u; listed += recs[t].stored; over += recs[t].count > RT_CROSS_LIST_MAX;
                    for (std::uint32_t j = 0; j < recs[t].stored; ++j)
                    {
                        const std::uint32_t a = object_of((std::uint32_t)t), b = object_of(members[t * RT_CROSS_LIST_MAX + j].primitive_id);
                        if (a != b) pairs.push_back({a < b ? a : b, a < b ? b : a});
                    }
                }
                std::sort(pairs.begin(), pairs.end());
                pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());
                std::cout << "self_cross: triangles " << nt << " crossing " << crossing << " listed " << listed << " above the list " << over << std::endl;
                for (const auto& p : pairs)
                {
                    std::cout << "self_cross   objects ";
                    print_object(p.first); std::cout << " | "; print_object(p.second);
                    std::cout << std::endl;
                }
            }
        };
        // --separation: one line per probe (rt_scene_separation through Render::Separation); --clearance: rt_scene_separation_self with
        // RT_SEPARATION_OTHER_OBJECTS over all triangles (Render::Clearance), reduced per ordered pair of objects as host.reduce_clearances reduces it
        auto print_separations = [&](bool objects_set)
        {
            for (const SeparationAt& q : separation_probes)
            {
                rt_separation rec;
                render.Separation(&q.probe, 1, q.r, &rec);
                std::cout << "separation " << q.probe.p1[0] << "," << q.probe.p1[1] << "," << q.probe.p1[2] << " " << q.probe.p2[0] << "," << q.probe.p2[1] << "," << q.probe.p2[2] << " "
                          << q.probe.p3[0] << "," << q.probe.p3[1] << "," << q.probe.p3[2] << ": ";
                if (!(rec.flags & RT_SEPARATION_SEARCHED)) { std::cout << "not searched" << std::endl; continue; }
                if (!(rec.flags & RT_SEPARATION_FOUND)) { std::cout << "none" << std::endl; continue; }
                std::cout << "distance " << rec.distance << ((rec.flags & RT_SEPARATION_CROSSING) ? " crossing" : "") << " primitive " << rec.primitive_id << " feature " << rec.feature
                          << " from " << rec.on_probe[0] << "," << rec.on_probe[1] << "," << rec.on_probe[2] << " to " << rec.on_scene[0] << "," << rec.on_scene[1] << "," << rec.on_scene[2]
                          << " object ";
                print_object(object_of(rec.primitive_id));
                std::cout << std::endl;
            }
            if (clearance)
            {
                const std::size_t nt = scene.GetTriangles().size(), n_objects = scene.GetObjectNames().size();
                if (!objects_set)                                              // rt_scene_set_objects wants a refittable upload: upload again, as the posing loop does
                {
                    render.GetIntegrator().SetRefittable(true);
                    render.UploadGPUData();
                }
                if (!objects_set) render.SetObjects(scene.GetTriangleObjects().data(), scene.GetTriangleObjects().size(), (std::uint32_t)n_objects);
                std::vector<rt_separation> recs(nt);
                render.Clearance(0u, nt, std::numeric_limits<float>::infinity(), recs.data());
                struct Key { float d; std::uint32_t t, u; bool operator<(const Key& o) const { return d < o.d || (d == o.d && (t < o.t || (t == o.t && u < o.u))); } };
                std::map<std::pair<std::uint32_t, std::uint32_t>, Key> best;                    // (object, other object) -> its nearest record
                for (std::size_t t = 0; t < nt; ++t)
                {
                    if (!(recs[t].flags & RT_SEPARATION_FOUND)) continue;
                    const std::pair<std::uint32_t, std::uint32_t> pair(object_of((std::uint32_t)t), object_of(recs[t].primitive_id));
                    const Key key = {recs[t].distance, (std::uint32_t)t, recs[t].primitive_id};
                    auto it = best.find(pair);
                    if (it == best.end() || key < it->second) best[pair] = key;
                }
                std::cout << "clearance: objects " << n_objects << " triangles " << nt << std::endl;
                for (std::uint32_t o = 0; o < n_objects; ++o)
                {
                    bool have = false, have_mine = true;
                    Key entry = {};
                    std::uint32_t other = 0u, record = 0u;
                    for (const auto& b : best)
                    {
                        if (b.first.first != o) continue;
                        const auto back = best.find({b.first.second, o});
                        const bool mine = back == best.end() || !(back->second.d < b.second.d);     // the smaller of the two directions
                        const Key e = mine ? b.second : Key{back->second.d, back->second.u, back->second.t};
                        if (!have || e < entry) { have = true; entry = e; other = b.first.second; record = mine ? e.t : e.u; have_mine = mine; }
                    }
                    std::cout << "clearance   ";
                    print_object(o);
                    std::cout << " | ";
                    if (!have) { std::cout << "none" << std::endl; continue; }
                    const rt_separation& r = recs[record];
                    const float* from = have_mine ? r.on_probe : r.on_scene;
                    const float* to = have_mine ? r.on_scene : r.on_probe;
                    print_object(other);
                    std::cout << " distance " << entry.d << ((r.flags & RT_SEPARATION_CROSSING) ? " crossing" : "") << " triangles " << entry.t << " " << entry.u << " from " << from[0] << ","
                              << from[1] << "," << from[2] << " to " << to[0] << "," << to[1] << "," << to[2] << std::endl;
                }
            }
        };
        // --pick_rect: one line per rectangle and one per object (rt_scene_select of the rectangle's region through Render::PickRect)
        auto print_pick_rects = [&]()
        {
            for (const RectAt& q : pick_rects)
            {
                std::vector<std::uint32_t> touching(scene.GetTriangles().size()), inside(scene.GetTriangles().size());
                render.PickRect(q.x0, q.y0, q.x1, q.y1, 0.0f, std::numeric_limits<float>::infinity(), nullptr, touching.data(), inside.data(), nullptr, nullptr);
                const std::size_t n_objects = scene.GetObjectNames().size();
                std::vector<std::uint32_t> any(n_objects, 0u), all(n_objects, 1u), has(n_objects, 0u);
                std::uint32_t count = 0u;
                for (std::size_t t = 0; t < touching.size(); ++t)
                {
                    const bool picked = ((q.window ? inside[t] : touching[t]) & 1u) != 0u;
                    count += picked ? 1u : 0u;
                    const std::uint32_t o = object_of((std::uint32_t)t);
                    if (o >= n_objects) continue;
                    has[o] = 1u;
                    any[o] |= touching[t] & 1u;
                    all[o] &= inside[t] & 1u;
                }
                std::cout << "pick_rect " << q.x0 << "," << q.y0 << " " << q.x1 << "," << q.y1 << (q.window ? " window" : "") << ": primitives " << count << std::endl;
                for (std::size_t o = 0; o < n_objects; ++o)
                    if (has[o] && (q.window ? all[o] : any[o]))
                    {
                        std::cout << "pick_rect   object ";
                        print_object((std::uint32_t)o);
                        std::cout << std::endl;
                    }
            }
        };
        // --ao: Render::OcclusionImage of the camera as it stands, written as a grey PFM
        auto write_ao = [&]()
        {
            if (ao_out.empty()) return;
            std::vector<float> grey((size_t)width * height), rgba((size_t)width * height * 4);
            render.OcclusionImage(ao, grey.data());
            for (size_t i = 0; i < grey.size(); ++i) { rgba[4 * i] = rgba[4 * i + 1] = rgba[4 * i + 2] = grey[i]; rgba[4 * i + 3] = 1.0f; }
            WritePFM(ao_out.c_str(), rgba, width, height);
            std::cout << "ambient occlusion (" << ao.samples << " rays per pixel, radius " << ao.radius << ") written to " << ao_out << std::endl;
        };
        // --ao_atlas / --lightmap: Render::OcclusionAtlas / IrradianceAtlas of the scene as it is posed, written as a grey / RGB PFM (row 0 = v 0 at the
        // bottom, as a texture is addressed)
        auto write_ao_atlas = [&]()
        {
            if (ao_atlas_out.empty() && lightmap_out.empty()) return;
            std::vector<float> uv;
            if (atlas_synthetic)                                              // scenes.synthetic_atlas: cell k = (k % columns, k / columns) holds triangles 2 k and 2 k + 1
            {
                const std::size_t nt = scene.GetTriangles().size(), cells = nt / 2 + nt % 2 > 0 ? nt / 2 + nt % 2 : 1;
                std::size_t columns = (std::size_t)std::ceil(std::sqrt((double)cells * (double)atlas.width / (double)(atlas.height ? atlas.height : 1u)));
                if (columns == 0) columns = 1;
                const std::size_t rows = (cells + columns - 1) / columns;
                uv.resize(nt * 6);
                for (std::size_t t = 0; t < nt; ++t)
                {
                    const std::size_t cx = (t / 2) % columns, cy = (t / 2) / columns;
                    const float u0 = (float)((double)cx / (double)columns), u1 = (float)((double)(cx + 1) / (double)columns);
                    const float v0 = (float)((double)cy / (double)rows), v1 = (float)((double)(cy + 1) / (double)rows);
                    const float first[6] = {u0, v0, u1, v0, u1, v1}, second[6] = {u0, v0, u1, v1, u0, v1};
                    for (int k = 0; k < 6; ++k) uv[t * 6 + k] = t % 2 == 0 ? first[k] : second[k];
                }
            }
            const bool sized = atlas.width >= 1u && atlas.height >= 1u && atlas.width <= 16384u && atlas.height <= 16384u && (std::uint64_t)atlas.width * atlas.height <= (1ull << 26);
            std::vector<float> grey(sized ? (size_t)atlas.width * atlas.height : 1u), rgba(grey.size() * 4);
            rt_atlas_stats st;
            if (!lightmap_out.empty())
            {
                rt_light_bake_desc lb;
                lb.samples = ao.samples; lb.seed = ao.seed; lb.flags = 0u; lb.bias = ao.bias; lb.sky_distance = RT_MAX_RENDER_DIST;
                std::vector<float> rgb(grey.size() * 3), turned(rgba.size());
                render.IrradianceAtlas(atlas, atlas_synthetic ? uv.data() : nullptr, lb, rgb.data(), &st);
                for (unsigned y = 0; y < atlas.height; ++y)
                    for (unsigned x = 0; x < atlas.width; ++x)
                    {
                        const float* s = &rgb[((size_t)(atlas.height - 1u - y) * atlas.width + x) * 3];
                        float* d = &turned[((size_t)y * atlas.width + x) * 4];
                        d[0] = s[0]; d[1] = s[1]; d[2] = s[2]; d[3] = 1.0f;
                    }
                WritePFM(lightmap_out.c_str(), turned, atlas.width, atlas.height);
                std::cout << "lightmap " << atlas.width << "x" << atlas.height << " (" << lb.samples << " sky rays per texel, sky + lights): covered " << st.covered
                          << " overlapped " << st.overlapped << " gutter " << st.gutter << " uncovered " << (size_t)atlas.width * atlas.height - st.covered - st.gutter
                          << " triangles_skipped " << st.triangles_skipped << " triangles_without_texel " << st.triangles_without_texel << " written to " << lightmap_out << std::endl;
            }
            if (ao_atlas_out.empty()) return;
            render.OcclusionAtlas(atlas, atlas_synthetic ? uv.data() : nullptr, ao, grey.data(), &st);
            for (size_t i = 0; i < grey.size(); ++i) { rgba[4 * i] = rgba[4 * i + 1] = rgba[4 * i + 2] = grey[i]; rgba[4 * i + 3] = 1.0f; }
            // (WritePFM puts the image's top row last; an atlas's row 0 is v = 0, the bottom of the texture: written first)
            std::vector<float> turned(rgba.size());
            for (unsigned y = 0; y < atlas.height; ++y)
                std::memcpy(&turned[(size_t)y * atlas.width * 4], &rgba[(size_t)(atlas.height - 1u - y) * atlas.width * 4], (size_t)atlas.width * 4 * sizeof(float));
            WritePFM(ao_atlas_out.c_str(), turned, atlas.width, atlas.height);
            std::cout << "ambient occlusion atlas " << atlas.width << "x" << atlas.height << " (" << ao.samples << " rays per texel, radius " << ao.radius << "): covered " << st.covered
                      << " overlapped " << st.overlapped << " gutter " << st.gutter << " uncovered " << (size_t)atlas.width * atlas.height - st.covered - st.gutter
                      << " triangles_skipped " << st.triangles_skipped << " triangles_without_texel " << st.triangles_without_texel << " written to " << ao_atlas_out << std::endl;
        };
        const bool posing = !object_steps.empty();
        if (posing)                                                           // effective at the loop's upload below
        {
            render.GetIntegrator().SetRefittable(true);
            if (temporal_iterations >= 0) render.GetIntegrator().SetRefitMotion(true);
        }
        if (moving || posing)
        {
            // the reference's moving-camera loop (Render::RenderFrame: a changed camera resets the frame): frame i is one sample at the start camera
            // moved by i * camera_step, resolved (and filtered) at its end
            render.UploadGPUData();
            render.GetIntegrator().SetResolveEveryFrame(true);
            render.GetIntegrator().SetSamplesAhead(samples_ahead);
            const std::size_t n_objects = scene.GetObjectNames().size();
            if (posing) render.SetObjects(scene.GetTriangleObjects().data(), scene.GetTriangleObjects().size(), (std::uint32_t)n_objects);
            std::vector<float> matrices(n_objects * 12, 0.0f);
            auto tf = std::chrono::steady_clock::now();
            for (unsigned i = 0; i < frames; ++i)
            {
                if (posing)                                                   // every object the identity, the stepped ones translated by i * step
                {
                    for (std::size_t k = 0; k < n_objects; ++k)
                    {
                        float* m = &matrices[k * 12];
                        for (int e = 0; e < 12; ++e) m[e] = 0.0f;
                        m[0] = m[5] = m[10] = 1.0f;
                    }
                    for (const ObjectStep& s : object_steps)
                        for (int a = 0; a < 3; ++a) matrices[(std::size_t)s.object * 12 + 4 * a + 3] += (float)i * s.d[a];
                    render.PoseObjects(matrices.data(), n_objects);
                }
                rt::Camera c = cam;
                c.position.x = cam.position.x + (float)i * camera_step[0];
                c.position.y = cam.position.y + (float)i * camera_step[1];
                c.position.z = cam.position.z + (float)i * camera_step[2];
                render.SetCamera(c);
                render.RenderFrame();
            }
            std::vector<float> const& img = render.GetIntegrator().GetResolvedImage();
            double df = std::chrono::duration<double>(std::chrono::steady_clock::now() - tf).count();
            std::cout << frames << (posing ? (moving ? " moving-camera, posed-object" : " posed-object") : " moving-camera") << " frames (one sample each" << (temporal_iterations >= 0 ? ", temporally filtered" : "") << ") in " << df
                      << " s: " << df * 1e3 / frames << " ms per frame" << std::endl;
            if (!out.empty()) WritePFM(out.c_str(), img, width, height);     // the last frame's resolved (filtered), tone-mapped image
            print_picks();
            print_picks_all();
            print_nearest();
            print_within();
            print_overlaps();
            print_crosses();
            print_separations(posing);
            print_pick_rects();
            write_ao();
            write_ao_atlas();
            return 0;
        }
        if (frames != 0)
        {
            // timing run: wait for the fold adaptation instead of adopting it whenever its worker is done (RT_CTX_OPT_ADAPTIVE_FOLD | 2, as bench.py does)
            if (rt_ctx_set_option(render.GetContext().Get(), RT_CTX_OPT_ADAPTIVE_FOLD, 27u) != RT_OK) throw rt::HIPException("rt_ctx_set_option failed");
            render.UploadGPUData();
            // The reference's main loop without its window (src/main.cpp:62-72 -> Render::RenderFrame, src/render.cpp:172-204): every frame is one
            // Integrate() through the hooks and ends with ResolveRadiance + Finish().  A warm-up batch first (the fold adaptation happens there),
            // then `frames` timed frames.  No Python, no PyTorch in this process: the HIP runtime is the system's.
            render.GetIntegrator().SetResolveEveryFrame(resolve);
            render.GetIntegrator().SetSamplesAhead(samples_ahead);
            render.RenderSamples(8);
            for (int i = 0; i < 24; ++i) render.RenderFrame();             // (the backend times its two ways over a scene's first 20 frames: RT_OPT_FRAME_KERNEL = 255)
            render.GetContext().Finish();
            rt_stats s0 = render.GetIntegrator().GetStats();
            auto tf = std::chrono::steady_clock::now();
            for (unsigned i = 0; i < frames; ++i) render.RenderFrame();
            (void)render.GetIntegrator().GetResolvedImage();               // the last image has arrived
            render.GetContext().Finish();
            double df = std::chrono::duration<double>(std::chrono::steady_clock::now() - tf).count();
            rt_stats s1 = render.GetIntegrator().GetStats();
            double frays = (double)(s1.closest_rays - s0.closest_rays) + (double)(s1.shadow_rays - s0.shadow_rays);
            // (RT_OPT_SAMPLES_AHEAD: the ray totals include the samples traced ahead at either end -- scaled to the timed frames' share; bench.py counts exactly)
            const double traced = (double)frames + (double)s1.samples_ahead - (double)s0.samples_ahead;
            if (traced > 0.0) frays *= (double)frames / traced;
            std::cout << frames << " frames (one Integrate() each, resolve + Finish() every frame) in " << df << " s: " << df * 1e3 / frames
                      << " ms per frame, " << frays / df / 1e6 << " Mrays/s (" << (s1.samples_from_banks - s0.samples_from_banks) << " of them replayed from batches traced ahead)" << std::endl;
            return 0;
        }
        auto t0 = std::chrono::steady_clock::now();
        render.RenderSamples(spp);
        render.GetContext().Finish();
        double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        rt_stats st = render.GetIntegrator().GetStats();
        double rays = (double)st.closest_rays + (double)st.shadow_rays;
        std::cout << spp << " spp in " << dt << " s, " << rays / dt / 1e6 << " Mrays/s" << std::endl;
        print_picks();
        print_picks_all();
        print_nearest();
        print_within();
        print_overlaps();
        print_crosses();
        print_separations(false);
        print_pick_rects();
        write_ao();
        write_ao_atlas();
        if (!out.empty() && (filter_iterations >= 0 || temporal_iterations >= 0))
            WritePFM(out.c_str(), render.GetIntegrator().ResolveNow(), width, height);     // the filtered, tone-mapped image
        else if (!out.empty())
        {
            std::vector<float> sum = render.GetIntegrator().ReadRadianceSum();
            for (float& v : sum) v /= (float)spp;
            WritePFM(out.c_str(), sum, width, height);
        }
    }
    catch (std::exception& ex)
    {
        std::cerr << "Caught exception: " << ex.what() << std::endl;   // main.cpp:74-77
        return 1;
    }
    return 0;
}
