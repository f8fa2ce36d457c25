/*
 * glref.c -- runs RayZen's OWN shaders (read at run time from /root/reference/RayZen/shaders/, never copied) on the
 * OpenGL implementation this image ships: Mesa 23.2 llvmpipe (swrast_dri.so), a conformant OpenGL 4.5 core software
 * renderer.  TEST INFRASTRUCTURE ONLY (the pin of oracle/rz_oracle.c; see oracle/glref/README.md): nothing in the product
 * path includes, links or runs it.
 *
 * The image has no X server, no EGL and no OSMesa, so there is no public way to ask for a context.  What it does have is the
 * driver itself and Mesa's own loader interface header (GL/internal/dri_interface.h, package mesa-common-dev): this file is
 * a DRI software-rasteriser LOADER -- the job libGLX_mesa / the X server do -- of ~100 lines: dlopen the driver, hand it
 * the swrast-loader callbacks (an off-screen drawable: nothing is ever presented), create a screen, a 4.3 core context
 * (RayZen's `#version 430 core`, src/main.cpp:215-217) and a dummy drawable, make it current, and fetch GL entry points
 * from Mesa's dispatch library (libglapi).  The GL implementation, the GLSL compiler and the rasteriser are Mesa's; nothing
 * of OpenGL is stood in for.
 *
 * What it replaces of the reference: the frame loop's draw (src/main.cpp:600-640): the SSBO uploads
 * (main.cpp:1072-1119, bindings 0,1,2,5,6,7,8,9), sendSceneDataToShader's uniforms (main.cpp:1356-1379, 1325-1343) and
 * glDrawArrays(GL_TRIANGLE_FAN, 0, 4) over the full-screen quad (main.cpp:1395-1409), into an RGBA32F colour attachment
 * instead of the window so that FragColor comes back unquantised.
 *
 * usage: glref <scene.blob> <out.f32> [shader_dir]
 *   scene.blob (little endian), written by oracle/glref/glref.py:
 *     char magic[4] = "RZGL"; int32 version = 2;
 *     int32 width, height, bounceBudget, numLights, numTriangles;
 *     int32 debugShowLights, debugShowBVH, debugBVHMode, debugSelectedBLAS, debugSelectedTri;
 *     int32 numSamples;   -- 1: the shader as it is.  N > 1: the ONE edit this harness can make to the text it loads --
 *                            FS:676's constant `int numSamples = 1; // increase for better quality` becomes N (the product
 *                            exposes that constant as `spp`); the fixtures say which they are
 *     float fps; float view[16], proj[16], invView[16], invProj[16]; float camPos[3];
 *     then 10 x { uint64 bytes; data }  -- the buffers of bindings 0..9 (bytes = 0: nothing is bound there)
 *   out.f32: width*height*4 floats, FragColor, row 0 = the bottom row (gl_FragCoord's origin).
 */
#define _GNU_SOURCE
#include <dlfcn.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <GL/glcorearb.h>
#include <GL/internal/dri_interface.h>

#define DIE(...) do { fprintf(stderr, "glref: " __VA_ARGS__); fprintf(stderr, "\n"); exit(2); } while (0)

/* ---- the swrast loader's callbacks: an off-screen drawable of 16 x 16 that is never shown ---- */
static void cb_get_drawable_info(__DRIdrawable* d, int* x, int* y, int* w, int* h, void* priv) { *x = 0; *y = 0; *w = 16; *h = 16; }
static void cb_put_image(__DRIdrawable* d, int op, int x, int y, int w, int h, char* data, void* priv) {}
static void cb_get_image(__DRIdrawable* d, int x, int y, int w, int h, char* data, void* priv) { memset(data, 0, (size_t)w * h * 4); }
static void cb_put_image2(__DRIdrawable* d, int op, int x, int y, int w, int h, int stride, char* data, void* priv) {}
static void cb_get_image2(__DRIdrawable* d, int x, int y, int w, int h, int stride, char* data, void* priv) { for (int r = 0; r < h; ++r) memset(data + (size_t)r * stride, 0, (size_t)w * 4); }

static const __DRIswrastLoaderExtension swrast_loader = {
    .base = {__DRI_SWRAST_LOADER, 3},
    .getDrawableInfo = cb_get_drawable_info,
    .putImage = cb_put_image,
    .getImage = cb_get_image,
    .putImage2 = cb_put_image2,
    .getImage2 = cb_get_image2,
};
static const __DRIextension* loader_extensions[] = {&swrast_loader.base, NULL};

static void* (*get_proc)(const char*);
#define GLFN(type, name) type name = (type)get_proc(#name); if (!name) DIE("no entry point %s", #name)

static char* read_text(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) DIE("cannot open %s", path);
    fseek(f, 0, SEEK_END);
    long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    char* s = malloc((size_t)n + 1);
    if (fread(s, 1, (size_t)n, f) != (size_t)n) DIE("short read of %s", path);
    s[n] = 0;
    fclose(f);
    return s;
}

typedef struct {
    char magic[4];
    int32_t version, width, height, bounceBudget, numLights, numTriangles;
    int32_t debugShowLights, debugShowBVH, debugBVHMode, debugSelectedBLAS, debugSelectedTri, numSamples;
    float fps, view[16], proj[16], invView[16], invProj[16], camPos[3];
} blob_header;

/* ---- Mesa's software driver, loaded the way libGLX_mesa loads it; a 4.3 core context made current ---- */
static void make_current(const char* driver) {
    void* drv = dlopen(driver, RTLD_NOW | RTLD_GLOBAL);
    if (!drv) DIE("dlopen %s: %s", driver, dlerror());
    const __DRIextension** (*get_ext)(void) = (const __DRIextension** (*)(void))dlsym(drv, __DRI_DRIVER_GET_EXTENSIONS "_swrast");
    if (!get_ext) DIE("driver has no %s_swrast", __DRI_DRIVER_GET_EXTENSIONS);
    const __DRIextension** exts = get_ext();
    const __DRIcoreExtension* core = NULL;
    const __DRIswrastExtension* swrast = NULL;
    for (int i = 0; exts[i]; ++i) {
        if (!strcmp(exts[i]->name, __DRI_CORE)) core = (const __DRIcoreExtension*)exts[i];
        if (!strcmp(exts[i]->name, __DRI_SWRAST)) swrast = (const __DRIswrastExtension*)exts[i];
    }
    if (!core || !swrast || swrast->base.version < 4) DIE("driver lacks DRI_Core / DRI_SWRast >= 4");
    const __DRIconfig** configs = NULL;
    __DRIscreen* screen = swrast->createNewScreen2(0, loader_extensions, exts, &configs, NULL);
    if (!screen || !configs || !configs[0]) DIE("createNewScreen2 failed");
    const uint32_t attribs[] = {__DRI_CTX_ATTRIB_MAJOR_VERSION, 4, __DRI_CTX_ATTRIB_MINOR_VERSION, 3};
    unsigned err = 0;
    __DRIcontext* ctx = swrast->createContextAttribs(screen, __DRI_API_OPENGL_CORE, configs[0], NULL, 2, attribs, &err, NULL);
    if (!ctx) DIE("no OpenGL 4.3 core context (error %u)", err);
    __DRIdrawable* draw = swrast->createNewDrawable(screen, configs[0], NULL);
    if (!draw) DIE("createNewDrawable failed");
    if (!core->bindContext(ctx, draw, draw)) DIE("bindContext failed");
    
    void* glapi = dlopen("libglapi.so.0", RTLD_NOW | RTLD_GLOBAL);
    if (!glapi) DIE("dlopen libglapi.so.0: %s", dlerror());
    get_proc = (void* (*)(const char*))dlsym(glapi, "_glapi_get_proc_address");
    if (!get_proc) DIE("no _glapi_get_proc_address");
}

/* ---- editor mode (blob magic "RZED"): RayZen's raster pass, buildRasterMeshes / sendRasterSceneData / renderRasterized
 * (main.cpp:1210-1297), with editor_vertex.glsl + editor_fragment.glsl read from shader_dir.
 *
 *   scene.blob (little endian), written by oracle/glref/glref.py: render_editor:
 *     char magic[4] = "RZED"; int32 version = 1;
 *     int32 width, height, numLights, nMeshes, nObjects;
 *     float view[16], proj[16], camPos[3], ambient[3], clear[4];
 *     uint64 bytes; materials (binding 1);  uint64 bytes; lights (binding 2)
 *     nMeshes x { int32 nVertices; nVertices x RasterVertex {float position[3], normal[3]; int32 materialIndex} }
 *     nObjects x { int32 mesh (-1: no mesh, skipped); float model[16]; float normalMatrix[9] }   -- gameObjects order
 *   out (row 0 = the bottom row): W*H x float[4] FragColor from an RGBA32F attachment; W*H x uint8[4] FragColor from an RGBA8
 *     attachment (the window's format); then the ID pass: W*H x int32[4] (object, gl_PrimitiveID, materialIndex, 1; -1 where
 *     nothing was drawn), W*H x float[4] (worldPos, gl_FragCoord.z), W*H x float[4] (the interpolated normal, 0);
 *     then W*H x uint32 the depth buffer (glReadPixels GL_UNSIGNED_INT).
 *   Each pass has its own framebuffer with a 24-bit depth renderbuffer (GLFW's default window depth), GL_LESS, cleared to
 *   1.0; no culling, no blending, no multisampling.  The ID pass runs the fragment shader named by GLREF_FRAGMENT (the
 *   harness's own oracle/glref/editor_ids.glsl) behind RayZen's editor_vertex.glsl; the harness fails unless all three
 *   passes leave bitwise-equal depth buffers, i.e. rasterised the same fragments. */
typedef struct {
    char magic[4];
    int32_t version, width, height, numLights, nMeshes, nObjects;
    float view[16], proj[16], camPos[3], ambient[3], clear[4];
} editor_header;

static void* read_sized(FILE* f, uint64_t* n) {
    if (fread(n, 8, 1, f) != 1) DIE("short blob");
    void* p = malloc(*n ? *n : 1);
    if (*n && fread(p, 1, *n, f) != *n) DIE("short blob");
    return p;
}

/* The ID pass's fragment shader (GLREF_FRAGMENT) holds the token GLREF_FRAGMENT_INPUTS once; it is replaced by the input
 * block that RayZen's editor_fragment.glsl declares -- from `in VS_OUT` through the block's closing `;`, which must occur
 * exactly once there -- so that the two fragment shaders read the same interface and no copy of it is kept here. */
static char* splice_inputs(const char* ids, const char* frag, const char* path) {
    const char* tok = "GLREF_FRAGMENT_INPUTS";
    const char* at = strstr(ids, tok);
    if (!at || strstr(at + 1, tok)) DIE("%s: expected exactly one %s", path, tok);
    const char* b = strstr(frag, "in VS_OUT");
    if (!b || strstr(b + 1, "in VS_OUT")) DIE("editor_fragment.glsl: expected exactly one input block `in VS_OUT`");
    const char* close = strchr(b, '}');
    const char* e = close ? strchr(close, ';') : NULL;
    if (!e) DIE("editor_fragment.glsl: the input block does not end");
    const size_t head = (size_t)(at - ids), block = (size_t)(e + 1 - b);
    char* out = malloc(strlen(ids) - strlen(tok) + block + 1);
    memcpy(out, ids, head);
    memcpy(out + head, b, block);
    strcpy(out + head + block, at + strlen(tok));
    return out;
}

static int editor_main(FILE* bf, const char* out_path, const char* shader_dir, const char* driver) {
    rewind(bf);
    editor_header H;
    if (fread(&H, sizeof H, 1, bf) != 1 || H.version != 1 || H.width <= 0 || H.height <= 0 || H.nMeshes < 0 || H.nObjects < 0)
        DIE("bad editor blob header");
    uint64_t matBytes, lightBytes;
    void* mats = read_sized(bf, &matBytes);
    void* lights = read_sized(bf, &lightBytes);
    int32_t* nVerts = calloc((size_t)H.nMeshes + 1, sizeof(int32_t));
    void** verts = calloc((size_t)H.nMeshes + 1, sizeof(void*));
    for (int m = 0; m < H.nMeshes; ++m) {
        if (fread(&nVerts[m], 4, 1, bf) != 1 || nVerts[m] < 0 || nVerts[m] % 3) DIE("bad mesh %d", m);
        verts[m] = malloc((size_t)nVerts[m] * 28 + 1);
        if (nVerts[m] && fread(verts[m], 28, (size_t)nVerts[m], bf) != (size_t)nVerts[m]) DIE("short blob (mesh %d)", m);
    }
    int32_t* objMesh = calloc((size_t)H.nObjects + 1, sizeof(int32_t));
    float* objModel = calloc((size_t)H.nObjects * 16 + 1, sizeof(float));
    float* objNormal = calloc((size_t)H.nObjects * 9 + 1, sizeof(float));
    for (int o = 0; o < H.nObjects; ++o) {
        if (fread(&objMesh[o], 4, 1, bf) != 1 || fread(objModel + 16 * o, 64, 1, bf) != 1 || fread(objNormal + 9 * o, 36, 1, bf) != 1)
            DIE("short blob (object %d)", o);
        if (objMesh[o] >= H.nMeshes) DIE("object %d: no mesh %d", o, objMesh[o]);
    }
    fclose(bf);

    make_current(driver);
    GLFN(PFNGLGETSTRINGPROC, glGetString);
    GLFN(PFNGLGETERRORPROC, glGetError);
    fprintf(stderr, "glref: %s | %s | GLSL %s\n", (const char*)glGetString(GL_RENDERER), (const char*)glGetString(GL_VERSION),
            (const char*)glGetString(GL_SHADING_LANGUAGE_VERSION));
    GLFN(PFNGLCREATESHADERPROC, glCreateShader);
    GLFN(PFNGLSHADERSOURCEPROC, glShaderSource);
    GLFN(PFNGLCOMPILESHADERPROC, glCompileShader);
    GLFN(PFNGLGETSHADERIVPROC, glGetShaderiv);
    GLFN(PFNGLGETSHADERINFOLOGPROC, glGetShaderInfoLog);
    GLFN(PFNGLCREATEPROGRAMPROC, glCreateProgram);
    GLFN(PFNGLATTACHSHADERPROC, glAttachShader);
    GLFN(PFNGLLINKPROGRAMPROC, glLinkProgram);
    GLFN(PFNGLGETPROGRAMIVPROC, glGetProgramiv);
    GLFN(PFNGLGETPROGRAMINFOLOGPROC, glGetProgramInfoLog);
    GLFN(PFNGLUSEPROGRAMPROC, glUseProgram);
    GLFN(PFNGLGETUNIFORMLOCATIONPROC, glGetUniformLocation);
    GLFN(PFNGLUNIFORM1IPROC, glUniform1i);
    GLFN(PFNGLUNIFORM3FVPROC, glUniform3fv);
    GLFN(PFNGLUNIFORMMATRIX3FVPROC, glUniformMatrix3fv);
    GLFN(PFNGLUNIFORMMATRIX4FVPROC, glUniformMatrix4fv);
    GLFN(PFNGLGENBUFFERSPROC, glGenBuffers);
    GLFN(PFNGLBINDBUFFERPROC, glBindBuffer);
    GLFN(PFNGLBUFFERDATAPROC, glBufferData);
    GLFN(PFNGLBINDBUFFERBASEPROC, glBindBufferBase);
    GLFN(PFNGLGENVERTEXARRAYSPROC, glGenVertexArrays);
    GLFN(PFNGLBINDVERTEXARRAYPROC, glBindVertexArray);
    GLFN(PFNGLVERTEXATTRIBPOINTERPROC, glVertexAttribPointer);
    GLFN(PFNGLVERTEXATTRIBIPOINTERPROC, glVertexAttribIPointer);
    GLFN(PFNGLENABLEVERTEXATTRIBARRAYPROC, glEnableVertexAttribArray);
    GLFN(PFNGLGENFRAMEBUFFERSPROC, glGenFramebuffers);
    GLFN(PFNGLBINDFRAMEBUFFERPROC, glBindFramebuffer);
    GLFN(PFNGLFRAMEBUFFERTEXTURE2DPROC, glFramebufferTexture2D);
    GLFN(PFNGLFRAMEBUFFERRENDERBUFFERPROC, glFramebufferRenderbuffer);
    GLFN(PFNGLGENRENDERBUFFERSPROC, glGenRenderbuffers);
    GLFN(PFNGLBINDRENDERBUFFERPROC, glBindRenderbuffer);
    GLFN(PFNGLRENDERBUFFERSTORAGEPROC, glRenderbufferStorage);
    GLFN(PFNGLCHECKFRAMEBUFFERSTATUSPROC, glCheckFramebufferStatus);
    GLFN(PFNGLGENTEXTURESPROC, glGenTextures);
    GLFN(PFNGLBINDTEXTUREPROC, glBindTexture);
    GLFN(PFNGLTEXIMAGE2DPROC, glTexImage2D);
    GLFN(PFNGLDRAWBUFFERSPROC, glDrawBuffers);
    GLFN(PFNGLVIEWPORTPROC, glViewport);
    GLFN(PFNGLCLEARCOLORPROC, glClearColor);
    GLFN(PFNGLCLEARDEPTHPROC, glClearDepth);
    GLFN(PFNGLCLEARPROC, glClear);
    GLFN(PFNGLCLEARBUFFERIVPROC, glClearBufferiv);
    GLFN(PFNGLCLEARBUFFERFVPROC, glClearBufferfv);
    GLFN(PFNGLDRAWARRAYSPROC, glDrawArrays);
    GLFN(PFNGLFINISHPROC, glFinish);
    GLFN(PFNGLREADPIXELSPROC, glReadPixels);
    GLFN(PFNGLREADBUFFERPROC, glReadBuffer);
    GLFN(PFNGLENABLEPROC, glEnable);
    GLFN(PFNGLDISABLEPROC, glDisable);
    GLFN(PFNGLDEPTHFUNCPROC, glDepthFunc);
    GLFN(PFNGLDEPTHMASKPROC, glDepthMask);
    GLFN(PFNGLCLAMPCOLORPROC, glClampColor);

    /* two programs: RayZen's (editor_vertex + editor_fragment) and the ID pass (editor_vertex + GLREF_FRAGMENT) */
    const char* idFrag = getenv("GLREF_FRAGMENT");
    if (!idFrag) DIE("editor mode needs GLREF_FRAGMENT (the ID pass's fragment shader)");
    GLuint progs[2];
    char path[4096];
    snprintf(path, sizeof path, "%s/editor_fragment.glsl", shader_dir);
    const char* editorFrag = read_text(path);
    for (int p = 0; p < 2; ++p) {
        progs[p] = glCreateProgram();
        for (int i = 0; i < 2; ++i) {
            if (i == 0) snprintf(path, sizeof path, "%s/editor_vertex.glsl", shader_dir);
            else if (p == 0) snprintf(path, sizeof path, "%s/editor_fragment.glsl", shader_dir);
            else snprintf(path, sizeof path, "%s", idFrag);
            const char* src = p == 0 && i == 1 ? editorFrag : read_text(path);
            if (p == 1 && i == 1) src = splice_inputs(src, editorFrag, path);
            GLuint sh = glCreateShader(i == 0 ? GL_VERTEX_SHADER : GL_FRAGMENT_SHADER);
            glShaderSource(sh, 1, &src, NULL);
            glCompileShader(sh);
            GLint ok = 0;
            glGetShaderiv(sh, GL_COMPILE_STATUS, &ok);
            if (!ok) { char log[8192]; glGetShaderInfoLog(sh, sizeof log, NULL, log); DIE("%s does not compile:\n%s", path, log); }
            glAttachShader(progs[p], sh);
        }
        glLinkProgram(progs[p]);
        GLint ok = 0;
        glGetProgramiv(progs[p], GL_LINK_STATUS, &ok);
        if (!ok) { char log[8192]; glGetProgramInfoLog(progs[p], sizeof log, NULL, log); DIE("link failed:\n%s", log); }
    }

    /* SSBOs 1 and 2 (main.cpp:1281-1282) */
    const void* ssbo[2] = {mats, lights};
    const uint64_t ssboBytes[2] = {matBytes, lightBytes};
    for (int b = 0; b < 2; ++b) {
        if (!ssboBytes[b]) continue;
        GLuint id;
        glGenBuffers(1, &id);
        glBindBuffer(GL_SHADER_STORAGE_BUFFER, id);
        glBufferData(GL_SHADER_STORAGE_BUFFER, (GLsizeiptr)ssboBytes[b], ssbo[b], GL_STATIC_DRAW);
        glBindBufferBase(GL_SHADER_STORAGE_BUFFER, (GLuint)(b + 1), id);
    }

    /* buildRasterMeshes (main.cpp:1210-1256): one VAO / VBO per non-empty mesh, the RasterVertex layout */
    GLuint* vao = calloc((size_t)H.nMeshes + 1, sizeof(GLuint));
    for (int m = 0; m < H.nMeshes; ++m) {
        if (!nVerts[m]) continue;
        GLuint vbo;
        glGenVertexArrays(1, &vao[m]);
        glGenBuffers(1, &vbo);
        glBindVertexArray(vao[m]);
        glBindBuffer(GL_ARRAY_BUFFER, vbo);
        glBufferData(GL_ARRAY_BUFFER, (GLsizeiptr)nVerts[m] * 28, verts[m], GL_STATIC_DRAW);
        glEnableVertexAttribArray(0);
        glVertexAttribPointer(0, 3, GL_FLOAT, GL_FALSE, 28, (void*)0);
        glEnableVertexAttribArray(1);
        glVertexAttribPointer(1, 3, GL_FLOAT, GL_FALSE, 28, (void*)12);
        glEnableVertexAttribArray(2);
        glVertexAttribIPointer(2, 1, GL_INT, 28, (void*)24);
        glBindVertexArray(0);
        glBindBuffer(GL_ARRAY_BUFFER, 0);
    }

    /* three framebuffers: colour RGBA32F, colour RGBA8, ID pass (RGBA32I + 2 x RGBA32F); each with a 24-bit depth buffer */
    const int W = H.width, Ht = H.height;
    const size_t n = (size_t)W * Ht;
    const GLenum fmts[3][3] = {{GL_RGBA32F, 0, 0}, {GL_RGBA8, 0, 0}, {GL_RGBA32I, GL_RGBA32F, GL_RGBA32F}};
    const GLenum bufs[3] = {GL_COLOR_ATTACHMENT0, GL_COLOR_ATTACHMENT1, GL_COLOR_ATTACHMENT2};
    GLuint fbo[3];
    uint32_t* depth[3];
    FILE* of = fopen(out_path, "wb");
    if (!of) DIE("cannot write %s", out_path);
    glViewport(0, 0, W, Ht);
    glClampColor(GL_CLAMP_READ_COLOR, GL_FALSE);
    glDisable(GL_CULL_FACE);
    glDisable(GL_BLEND);
    glDisable(GL_MULTISAMPLE);
    for (int pass = 0; pass < 3; ++pass) {
        glGenFramebuffers(1, &fbo[pass]);
        glBindFramebuffer(GL_FRAMEBUFFER, fbo[pass]);
        const int nAtt = pass == 2 ? 3 : 1;
        for (int a = 0; a < nAtt; ++a) {
            GLuint tex;
            glGenTextures(1, &tex);
            glBindTexture(GL_TEXTURE_2D, tex);
            const GLenum f = fmts[pass][a];
            glTexImage2D(GL_TEXTURE_2D, 0, f, W, Ht, 0, f == GL_RGBA32I ? GL_RGBA_INTEGER : GL_RGBA,
                         f == GL_RGBA32I ? GL_INT : f == GL_RGBA8 ? GL_UNSIGNED_BYTE : GL_FLOAT, NULL);
            glFramebufferTexture2D(GL_FRAMEBUFFER, bufs[a], GL_TEXTURE_2D, tex, 0);
        }
        GLuint rb;
        glGenRenderbuffers(1, &rb);
        glBindRenderbuffer(GL_RENDERBUFFER, rb);
        glRenderbufferStorage(GL_RENDERBUFFER, GL_DEPTH_COMPONENT24, W, Ht);
        glFramebufferRenderbuffer(GL_FRAMEBUFFER, GL_DEPTH_ATTACHMENT, GL_RENDERBUFFER, rb);
        glDrawBuffers(nAtt, bufs);
        if (glCheckFramebufferStatus(GL_FRAMEBUFFER) != GL_FRAMEBUFFER_COMPLETE) DIE("framebuffer %d incomplete", pass);

        /* renderRasterized (main.cpp:1259-1297) */
        glEnable(GL_DEPTH_TEST);
        glDepthFunc(GL_LESS);
        glDepthMask(GL_TRUE);
        glClearDepth(1.0);
        if (pass < 2) {
            glClearColor(H.clear[0], H.clear[1], H.clear[2], H.clear[3]);
            glClear(GL_COLOR_BUFFER_BIT | GL_DEPTH_BUFFER_BIT);
        } else {
            const GLint none[4] = {-1, -1, -1, -1};
            const GLfloat zero[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            glClearBufferiv(GL_COLOR, 0, none);
            glClearBufferfv(GL_COLOR, 1, zero);
            glClearBufferfv(GL_COLOR, 2, zero);
            glClear(GL_DEPTH_BUFFER_BIT);
        }
        const GLuint prog = progs[pass == 2];
        glUseProgram(prog);
        glUniformMatrix4fv(glGetUniformLocation(prog, "uView"), 1, GL_FALSE, H.view);
        glUniformMatrix4fv(glGetUniformLocation(prog, "uProj"), 1, GL_FALSE, H.proj);
        glUniform3fv(glGetUniformLocation(prog, "uCameraPos"), 1, H.camPos);
        glUniform1i(glGetUniformLocation(prog, "numLights"), H.numLights);
        glUniform3fv(glGetUniformLocation(prog, "uAmbientColor"), 1, H.ambient);
        const GLint modelLoc = glGetUniformLocation(prog, "uModel"), normalLoc = glGetUniformLocation(prog, "uNormalMatrix");
        const GLint objLoc = glGetUniformLocation(prog, "uObjectIndex");
        for (int o = 0; o < H.nObjects; ++o) {
            const int m = objMesh[o];
            if (m < 0 || !nVerts[m]) continue;
            glUniformMatrix4fv(modelLoc, 1, GL_FALSE, objModel + 16 * o);
            glUniformMatrix3fv(normalLoc, 1, GL_FALSE, objNormal + 9 * o);
            if (objLoc >= 0) glUniform1i(objLoc, o);
            glBindVertexArray(vao[m]);
            glDrawArrays(GL_TRIANGLES, 0, nVerts[m]);
        }
        glBindVertexArray(0);
        glUseProgram(0);
        glFinish();

        for (int a = 0; a < nAtt; ++a) {
            const GLenum f = fmts[pass][a];
            const size_t px = f == GL_RGBA8 ? 4 : 16;
            void* buf = malloc(n * px);
            glReadBuffer(bufs[a]);
            glReadPixels(0, 0, W, Ht, f == GL_RGBA32I ? GL_RGBA_INTEGER : GL_RGBA,
                         f == GL_RGBA32I ? GL_INT : f == GL_RGBA8 ? GL_UNSIGNED_BYTE : GL_FLOAT, buf);
            if (fwrite(buf, px, n, of) != n) DIE("cannot write %s", out_path);
            free(buf);
        }
        depth[pass] = malloc(n * 4);
        glReadPixels(0, 0, W, Ht, GL_DEPTH_COMPONENT, GL_UNSIGNED_INT, depth[pass]);
        const GLenum e = glGetError();
        if (e != GL_NO_ERROR) DIE("GL error 0x%x in pass %d", e, pass);
        if (pass > 0 && memcmp(depth[pass], depth[0], n * 4)) DIE("pass %d left another depth buffer than the colour pass", pass);
    }
    if (fwrite(depth[0], 4, n, of) != n) DIE("cannot write %s", out_path);
    fclose(of);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 3) DIE("usage: glref <scene.blob> <out.f32> [shader_dir]");
    const char* shader_dir = argc > 3 ? argv[3] : "/root/reference/RayZen/shaders";
    const char* driver = getenv("GLREF_DRIVER") ? getenv("GLREF_DRIVER") : "/usr/lib/x86_64-linux-gnu/dri/swrast_dri.so";

    /* ---- the scene ---- */
    FILE* bf = fopen(argv[1], "rb");
    if (!bf) DIE("cannot open %s", argv[1]);
    char magic[4];
    if (fread(magic, 4, 1, bf) != 1) DIE("short blob");
    if (!memcmp(magic, "RZED", 4)) return editor_main(bf, argv[2], shader_dir, driver);
    rewind(bf);
    blob_header H;
    if (fread(&H, sizeof H, 1, bf) != 1 || memcmp(H.magic, "RZGL", 4) != 0 || H.version != 2) DIE("bad blob header");
    void* bufs[10];
    uint64_t bytes[10];
    for (int b = 0; b < 10; ++b) {
        if (fread(&bytes[b], 8, 1, bf) != 1) DIE("short blob");
        bufs[b] = malloc(bytes[b] ? bytes[b] : 1);
        if (bytes[b] && fread(bufs[b], 1, bytes[b], bf) != bytes[b]) DIE("short blob (binding %d)", b);
    }
    fclose(bf);

    make_current(driver);

    GLFN(PFNGLGETSTRINGPROC, glGetString);
    GLFN(PFNGLGETERRORPROC, glGetError);
    fprintf(stderr, "glref: %s | %s | GLSL %s\n", (const char*)glGetString(GL_RENDERER), (const char*)glGetString(GL_VERSION),
            (const char*)glGetString(GL_SHADING_LANGUAGE_VERSION));
    if (getenv("GLREF_PROBE")) return 0;

    GLFN(PFNGLCREATESHADERPROC, glCreateShader);
    GLFN(PFNGLSHADERSOURCEPROC, glShaderSource);
    GLFN(PFNGLCOMPILESHADERPROC, glCompileShader);
    GLFN(PFNGLGETSHADERIVPROC, glGetShaderiv);
    GLFN(PFNGLGETSHADERINFOLOGPROC, glGetShaderInfoLog);
    GLFN(PFNGLCREATEPROGRAMPROC, glCreateProgram);
    GLFN(PFNGLATTACHSHADERPROC, glAttachShader);
    GLFN(PFNGLLINKPROGRAMPROC, glLinkProgram);
    GLFN(PFNGLGETPROGRAMIVPROC, glGetProgramiv);
    GLFN(PFNGLGETPROGRAMINFOLOGPROC, glGetProgramInfoLog);
    GLFN(PFNGLUSEPROGRAMPROC, glUseProgram);
    GLFN(PFNGLGETUNIFORMLOCATIONPROC, glGetUniformLocation);
    GLFN(PFNGLUNIFORM1IPROC, glUniform1i);
    GLFN(PFNGLUNIFORM1FPROC, glUniform1f);
    GLFN(PFNGLUNIFORM2FPROC, glUniform2f);
    GLFN(PFNGLUNIFORM3FVPROC, glUniform3fv);
    GLFN(PFNGLUNIFORMMATRIX4FVPROC, glUniformMatrix4fv);
    GLFN(PFNGLGENBUFFERSPROC, glGenBuffers);
    GLFN(PFNGLBINDBUFFERPROC, glBindBuffer);
    GLFN(PFNGLBUFFERDATAPROC, glBufferData);
    GLFN(PFNGLBINDBUFFERBASEPROC, glBindBufferBase);
    GLFN(PFNGLGENVERTEXARRAYSPROC, glGenVertexArrays);
    GLFN(PFNGLBINDVERTEXARRAYPROC, glBindVertexArray);
    GLFN(PFNGLVERTEXATTRIBPOINTERPROC, glVertexAttribPointer);
    GLFN(PFNGLENABLEVERTEXATTRIBARRAYPROC, glEnableVertexAttribArray);
    GLFN(PFNGLGENFRAMEBUFFERSPROC, glGenFramebuffers);
    GLFN(PFNGLBINDFRAMEBUFFERPROC, glBindFramebuffer);
    GLFN(PFNGLFRAMEBUFFERTEXTURE2DPROC, glFramebufferTexture2D);
    GLFN(PFNGLCHECKFRAMEBUFFERSTATUSPROC, glCheckFramebufferStatus);
    GLFN(PFNGLGENTEXTURESPROC, glGenTextures);
    GLFN(PFNGLBINDTEXTUREPROC, glBindTexture);
    GLFN(PFNGLTEXIMAGE2DPROC, glTexImage2D);
    GLFN(PFNGLVIEWPORTPROC, glViewport);
    GLFN(PFNGLCLEARCOLORPROC, glClearColor);
    GLFN(PFNGLCLEARPROC, glClear);
    GLFN(PFNGLDRAWARRAYSPROC, glDrawArrays);
    GLFN(PFNGLFINISHPROC, glFinish);
    GLFN(PFNGLREADPIXELSPROC, glReadPixels);
    GLFN(PFNGLREADBUFFERPROC, glReadBuffer);
    GLFN(PFNGLDISABLEPROC, glDisable);
    GLFN(PFNGLCLAMPCOLORPROC, glClampColor);

    /* ---- RayZen's program, from RayZen's files ---- */
    char path[4096];
    GLuint sh[2];
    const char* names[2] = {"vertex_shader.glsl", "fragment_shader.glsl"};
    const GLenum kinds[2] = {GL_VERTEX_SHADER, GL_FRAGMENT_SHADER};
    GLuint prog = glCreateProgram();
    for (int i = 0; i < 2; ++i) {
        snprintf(path, sizeof path, "%s/%s", shader_dir, names[i]);
        /* GLREF_FRAGMENT: another fragment shader behind the same interface -- oracle/glref/probe_math.glsl, which tabulates
         * llvmpipe's sin / cos / acos / pow so that the tests can tell its built-ins from the oracle's (never used for a frame) */
        if (i == 1 && getenv("GLREF_FRAGMENT")) snprintf(path, sizeof path, "%s", getenv("GLREF_FRAGMENT"));
        const char* src = read_text(path);
        if (i == 1 && H.numSamples > 1) {       /* FS:676's constant, see the header comment */
            const char* key = "int numSamples = 1;";
            char* at = strstr(src, key);
            if (!at || strstr(at + 1, key)) DIE("%s: expected exactly one `%s`", path, key);
            char* patched = malloc(strlen(src) + 32);
            const int head = (int)(at - src);
            sprintf(patched, "%.*sint numSamples = %d;%s", head, src, H.numSamples, at + strlen(key));
            src = patched;
        }
        sh[i] = glCreateShader(kinds[i]);
        glShaderSource(sh[i], 1, &src, NULL);
        glCompileShader(sh[i]);
        GLint ok = 0;
        glGetShaderiv(sh[i], GL_COMPILE_STATUS, &ok);
        if (!ok) { char log[8192]; glGetShaderInfoLog(sh[i], sizeof log, NULL, log); DIE("%s does not compile:\n%s", path, log); }
        glAttachShader(prog, sh[i]);
    }
    glLinkProgram(prog);
    { GLint ok = 0; glGetProgramiv(prog, GL_LINK_STATUS, &ok); if (!ok) { char log[8192]; glGetProgramInfoLog(prog, sizeof log, NULL, log); DIE("link failed:\n%s", log); } }
    glUseProgram(prog);

    /* ---- uniforms (main.cpp:1356-1379, 1325-1343, 625-633) ---- */
    glUniform2f(glGetUniformLocation(prog, "resolution"), (float)H.width, (float)H.height);
    glUniform1i(glGetUniformLocation(prog, "numTriangles"), H.numTriangles);
    glUniform1i(glGetUniformLocation(prog, "numLights"), H.numLights);
    glUniform1i(glGetUniformLocation(prog, "uniformBounceBudget"), H.bounceBudget);
    glUniformMatrix4fv(glGetUniformLocation(prog, "camera.viewMatrix"), 1, GL_FALSE, H.view);
    glUniformMatrix4fv(glGetUniformLocation(prog, "camera.projectionMatrix"), 1, GL_FALSE, H.proj);
    glUniform3fv(glGetUniformLocation(prog, "camera.position"), 1, H.camPos);
    glUniformMatrix4fv(glGetUniformLocation(prog, "camera.invViewMatrix"), 1, GL_FALSE, H.invView);
    glUniformMatrix4fv(glGetUniformLocation(prog, "camera.invProjectionMatrix"), 1, GL_FALSE, H.invProj);
    glUniform1i(glGetUniformLocation(prog, "debugShowLights"), H.debugShowLights);
    glUniform1i(glGetUniformLocation(prog, "debugShowBVH"), H.debugShowBVH);
    glUniform1i(glGetUniformLocation(prog, "debugBVHMode"), H.debugBVHMode);
    glUniform1i(glGetUniformLocation(prog, "debugSelectedBLAS"), H.debugSelectedBLAS);
    glUniform1i(glGetUniformLocation(prog, "debugSelectedTri"), H.debugSelectedTri);
    glUniform1f(glGetUniformLocation(prog, "uniformFps"), H.fps);

    /* ---- SSBOs (main.cpp:1072-1119) ---- */
    for (int b = 0; b < 10; ++b) {
        if (!bytes[b]) continue;
        GLuint id;
        glGenBuffers(1, &id);
        glBindBuffer(GL_SHADER_STORAGE_BUFFER, id);
        glBufferData(GL_SHADER_STORAGE_BUFFER, (GLsizeiptr)bytes[b], bufs[b], GL_STATIC_DRAW);
        glBindBufferBase(GL_SHADER_STORAGE_BUFFER, (GLuint)b, id);
    }

    /* ---- the quad (main.cpp:1395-1409) and an RGBA32F target ---- */
    const float quad[12] = {-1.0f, -1.0f, 0.0f, 1.0f, -1.0f, 0.0f, 1.0f, 1.0f, 0.0f, -1.0f, 1.0f, 0.0f};
    GLuint vao, vbo, fbo, tex;
    glGenVertexArrays(1, &vao);
    glBindVertexArray(vao);
    glGenBuffers(1, &vbo);
    glBindBuffer(GL_ARRAY_BUFFER, vbo);
    glBufferData(GL_ARRAY_BUFFER, sizeof quad, quad, GL_STATIC_DRAW);
    glVertexAttribPointer(0, 3, GL_FLOAT, GL_FALSE, 3 * sizeof(float), (void*)0);
    glEnableVertexAttribArray(0);
    glGenTextures(1, &tex);
    glBindTexture(GL_TEXTURE_2D, tex);
    glTexImage2D(GL_TEXTURE_2D, 0, GL_RGBA32F, H.width, H.height, 0, GL_RGBA, GL_FLOAT, NULL);
    glGenFramebuffers(1, &fbo);
    glBindFramebuffer(GL_FRAMEBUFFER, fbo);
    glFramebufferTexture2D(GL_FRAMEBUFFER, GL_COLOR_ATTACHMENT0, GL_TEXTURE_2D, tex, 0);
    if (glCheckFramebufferStatus(GL_FRAMEBUFFER) != GL_FRAMEBUFFER_COMPLETE) DIE("framebuffer incomplete");
    glViewport(0, 0, H.width, H.height);
    glDisable(GL_DEPTH_TEST);
    glDisable(GL_BLEND);
    glClampColor(GL_CLAMP_READ_COLOR, GL_FALSE);
    glClearColor(0.0f, 0.0f, 0.0f, 0.0f);
    glClear(GL_COLOR_BUFFER_BIT);
    glDrawArrays(GL_TRIANGLE_FAN, 0, 4);
    glFinish();
    float* out = malloc((size_t)H.width * H.height * 16);
    glReadBuffer(GL_COLOR_ATTACHMENT0);
    glReadPixels(0, 0, H.width, H.height, GL_RGBA, GL_FLOAT, out);
    const GLenum e = glGetError();
    if (e != GL_NO_ERROR) DIE("GL error 0x%x", e);
    FILE* of = fopen(argv[2], "wb");
    if (!of || fwrite(out, 16, (size_t)H.width * H.height, of) != (size_t)H.width * H.height) DIE("cannot write %s", argv[2]);
    fclose(of);
    return 0;
}
